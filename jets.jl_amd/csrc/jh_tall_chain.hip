// jh_tall_chain.hip -- the chain handle and the C ABI of the fused chains (jh_chain_*); the kernels and their launchers live in jh_tall_chain_kernels.h and are
// instantiated in three translation units (this one: FORWARD; jh_tall_chain_adj.hip: ADJOINT; jh_tall_chain_nrm.hip: NORMAL) -- one unit took 104 s to
// compile, the critical path of every build.
#include "jh_tall_chain_kernels.h"

namespace jhb {
// the domain's elements [first_elem, end_elem) (not scalars: a complex element counts once)
// (ca: another program over the handle's rows and streams -- a FORWARD chain's derived ADJOINT / NORMAL program; NULL: the handle's own)
int chain_launch_adjoint(const jh_chain *ch, void *out, const void *in, int accumulate, int64_t first_elem, int64_t end_elem, const ChainArgs *ca = nullptr);   // jh_tall_chain_adj.hip
int chain_launch_normal(const jh_chain *ch, void *out, const void *in, int accumulate, int64_t first_elem, int64_t end_elem, const ChainArgs *ca = nullptr);    // jh_tall_chain_nrm.hip
int chain_launch_step(const jh_chain *ch, const ChainArgs &ca, void *u, const void *v, void *w, double alpha, double beta, double *normsq,
                      int64_t first_elem, int64_t end_elem, bool defer);                                      // jh_tall_chain_step.hip
bool grid_chain_ok(const jh_blockop *op);                                                                     // jh_grid_chain.hip
bool grid_chain_vectors_ok(const jh_blockop *op, const void *a, const void *b);
int grid_chain_launch(const jh_chain *ch, int prog, int type, void *out, const void *in, int accumulate);   // prog: 0 own, 1 / 2 the derived ADJOINT / NORMAL
int grid_chain_launch_range(const jh_chain *ch, void *out, const void *in, int accumulate, int64_t first_elem, int64_t count);   // an ADJOINT / NORMAL handle's own program over positions inside a block
}  // namespace jhb

namespace {

// one side's stages -> its program; DIAG stages get a stream each unless they name an array the side already streams
int build_prog(const char *side, int n, const jh_chain_stage *st, int dtype, int64_t nrow_ptrs, ChainProg &p, std::vector<const jh_chain_stage *> &streams)
{
    JH_REQUIRE(n >= 0 && n <= JH_CHAIN_MAX_STAGES, "jh_chain_create: %d %s stages (at most %d)", n, side, JH_CHAIN_MAX_STAGES);
    JH_REQUIRE(n == 0 || st, "jh_chain_create: null %s stage list", side);
    const bool wide_ok = dtype == JH_F32 || dtype == JH_C32;
    for (int s = 0; s < JH_CHAIN_MAX_STAGES; s++) { p.st[s] = CK_NONE; p.a32[s] = 0.f; p.a[s] = 0.0; }
    for (int s = 0; s < n; s++) {
        const jh_chain_stage &g = st[s];
        if (g.kind == JH_STAGE_SCALE) {
            JH_REQUIRE((g.flags & ~(JH_SCALAR_COMPLEX | JH_SCALAR_WIDE)) == 0, "jh_chain_create: unknown flags %d on a SCALE stage", g.flags);
            if (g.flags & JH_SCALAR_COMPLEX) return jh_fail(JH_ERR_UNSUPPORTED, "jh_chain_create: a Complex scalar takes the stage-by-stage chain");
            const bool wide = (g.flags & JH_SCALAR_WIDE) && wide_ok;
            p.st[s] = wide ? CK_SCALE_WIDE : CK_SCALE;
            p.a[s] = g.a;
            p.a32[s] = (float)g.a;
        } else if (g.kind == JH_STAGE_DIAG) {
            JH_REQUIRE((g.flags & ~(JH_STAGE_CONJ | JH_STAGE_ROWSUM)) == 0, "jh_chain_create: unknown flags %d on a DIAG stage", g.flags);
            JH_REQUIRE(!(g.flags & JH_STAGE_ROWSUM) || g.row_flags, "jh_chain_create: JH_STAGE_ROWSUM is for the children of a block-diagonal block operator (range side, row_flags given)");
            JH_REQUIRE(g.coeff, "jh_chain_create: a DIAG stage without coefficient pointers");
            int found = -1;
            for (size_t q = 0; q < streams.size() && found < 0; q++) {
                bool same = (streams[q]->row_flags == nullptr) == (g.row_flags == nullptr);
                for (int64_t i = 0; i < nrow_ptrs && same; i++)
                    same = streams[q]->coeff[i] == g.coeff[i] && (!g.row_flags || streams[q]->row_flags[i] == g.row_flags[i]);
                if (same) found = (int)q;
            }
            if (found < 0) {
                if ((int)streams.size() >= JH_CHAIN_MAX_STREAMS)
                    return jh_fail(JH_ERR_UNSUPPORTED, "jh_chain_create: more than %d coefficient arrays on the %s side", JH_CHAIN_MAX_STREAMS, side);
                found = (int)streams.size();
                streams.push_back(&g);
            }
            p.st[s] = (uint32_t)((g.flags & JH_STAGE_CONJ) ? CK_DIAG_CONJ : CK_DIAG) | ((uint32_t)found << 4) | ((g.flags & JH_STAGE_ROWSUM) ? CK_ROWSUM : 0u);
        } else {
            return jh_fail(JH_ERR_INVALID, "jh_chain_create: unknown stage kind %d", g.kind);
        }
    }
    return JH_OK;
}

// the adjoint of a stage list: the stages in reverse order, each its own adjoint -- a real scalar is itself (conj(a) == a, src/Jets.jl:1160), a
// diagonal its conjugate (the same array and stream; a row's own conj flag and a block operator's ROWSUM stay: the kernel flips per row).  `at`:
// where in `out` they go.  Returns the number of stages.
int adjoint_prog(const ChainProg &in, ChainProg &out, int at)
{
    int n = 0;
    while (n < JH_CHAIN_MAX_STAGES && (in.st[n] & 15u) != CK_NONE) n++;
    for (int s = 0; s < n && at + s < JH_CHAIN_MAX_STAGES; s++) {
        const int from = n - 1 - s;
        uint32_t w = in.st[from];
        const uint32_t k = w & 15u;
        if (k == CK_DIAG || k == CK_DIAG_CONJ) w = (w & ~15u) | (k == CK_DIAG ? CK_DIAG_CONJ : CK_DIAG);
        out.st[at + s] = w;
        out.a32[at + s] = in.a32[from];
        out.a[at + s] = in.a[from];
    }
    return n;
}

// the ADJOINT, NORMAL and step programs of a FORWARD chain (jh_chain::adj_args, nrm_args, step_args)
void derive_progs(jh_chain *ch)
{
    const ChainArgs &f = ch->args;
    ChainArgs adj{}, nrm{};
    for (int s = 0; s < JH_CHAIN_MAX_STAGES; s++) adj.pre.st[s] = adj.mid.st[s] = adj.post.st[s] = nrm.mid.st[s] = nrm.post.st[s] = CK_NONE;
    adj.rows = nrm.rows = f.rows;
    (void)adjoint_prog(f.mid, adj.mid, 0);
    (void)adjoint_prog(f.pre, adj.post, 0);
    for (int q = 0; q < JH_CHAIN_MAX_STREAMS; q++) adj.post_c[q] = nrm.post_c[q] = nrm.pre_c[q] = f.pre_c[q];
    nrm.pre = f.pre;
    nrm.mid = f.mid;
    nrm.post = adj.post;
    int nr = 0;
    while (nr < JH_CHAIN_MAX_STAGES && (f.mid.st[nr] & 15u) != CK_NONE) nr++;
    ch->nrm_ok = 2 * nr <= JH_CHAIN_MAX_STAGES;
    if (ch->nrm_ok) (void)adjoint_prog(f.mid, nrm.mid, nr);
    ChainArgs stp = nrm;                     // the step: R alone in the range-side list (k_chain_adj MODE 2 applies R^H from it, mid_step)
    stp.mid = f.mid;
    ch->step_args = stp;
    ch->adj_args = adj;
    ch->nrm_args = nrm;
}

// are the vectors (and the operator's coefficients) aligned as the chain's kernels need them?  (NULL: not checked)
bool chain_vectors_ok(const jh_chain *ch, const void *rng, const void *dom)
{
    return ch->ncol > 1 ? jhb::grid_chain_vectors_ok(ch->op, rng, dom) : jhb::tall_unaligned_ok(ch->op, rng, dom);
}

// word 0 (a grid: words 0 .. K-1) of every record from the operator's blocks as they are NOW, then the table to the device (at create, and again when jh_blockop_point has
// moved the SQUARE rows' arrays since)
int chain_sync_rows(jh_chain *ch)
{
    const jh_blockop *op = ch->op;
    const size_t rw = (size_t)(ch->ncol + ch->nw);
    for (int64_t i = 0; i < op->nrow; i++)
        for (int k = 0; k < ch->ncol; k++) {
            const jh_block_desc &b = op->blocks[(size_t)(i + k * op->nrow)];             // (the block table is column-major)
            const jh_dev_block db = jh_dev_block_of(b);
            const uint64_t p = (uint64_t)(uintptr_t)(ch->ncol == 1 || b.kind == JH_OP_DIAG ? b.coeff : nullptr);
            JH_REQUIRE((p >> 48) == 0, "fused chain: a coefficient address does not fit 48 bits");
            ch->host_tab[(size_t)i * rw + (size_t)k] = p | ((uint64_t)(b.kind & 7) << 48) | ((uint64_t)(b.adjoint ? 1 : 0) << 51) | ((uint64_t)(db.real_scale ? 1 : 0) << 52);
        }
    JH_CHECK_HIP(hipMemcpyAsync(ch->dev_tab, ch->host_tab.data(), ch->host_tab.size() * sizeof(uint64_t), hipMemcpyHostToDevice, jh_ctx().stream));
    JH_CHECK_HIP(hipStreamSynchronize(jh_ctx().stream));
    ch->op_gen = op->table_gen;
    return JH_OK;
}

// the checks every application of a chain makes (whole-vector or ranged): arguments, lengths, aliasing, the linearisation point, alignment
int chain_check(const jh_chain *ch, const jh_bvec *out, const jh_bvec *x, int accumulate, const char *fn)
{
    const jh_blockop *op = ch->op;
    JH_REQUIRE(accumulate >= -2 && accumulate <= 2, "%s: accumulate must be 0, +-1 or +-2 (got %d)", fn, accumulate);
    JH_REQUIRE(out->dtype == op->dtype && x->dtype == op->dtype, "%s: dtype mismatch", fn);
    const int64_t nrange = op->row_off[(size_t)op->nrow], ndom = op->col_off[(size_t)op->ncol];
    const int64_t want_out = ch->type == JH_CHAIN_FORWARD ? nrange : ndom, want_in = ch->type == JH_CHAIN_ADJOINT ? nrange : ndom;
    JH_REQUIRE(out->length == want_out && x->length == want_in, "%s: vectors have %lld / %lld elements, the chain maps %lld -> %lld", fn,
               (long long)out->length, (long long)x->length, (long long)want_in, (long long)want_out);
    JH_REQUIRE(out->data != x->data, "%s: the output must not alias the input", fn);
    if (op->nonlinear && !op->pointed)
        return jh_fail(JH_ERR_STATE, "%s: operator has nonlinear blocks and no linearisation point (jh_blockop_point)", fn);
    const void *rng = ch->type == JH_CHAIN_FORWARD ? out->data : (ch->type == JH_CHAIN_ADJOINT ? x->data : nullptr);
    const void *dom = ch->type == JH_CHAIN_FORWARD ? x->data : out->data;
    if (!chain_vectors_ok(ch, rng, dom) || (ch->type == JH_CHAIN_NORMAL && !chain_vectors_ok(ch, nullptr, x->data)))
        return jh_fail(JH_ERR_UNSUPPORTED, "%s: a vector or coefficient array is not aligned like its scalar", fn);
    return JH_OK;
}

}  // namespace

extern "C" {

int jh_chain_create(const jh_blockop *op, int type, int npre, const jh_chain_stage *pre, int nmid, const jh_chain_stage *mid, int npost,
                    const jh_chain_stage *post, jh_chain **out)
{
    JH_TRY(jh_enter(op));
    JH_REQUIRE(op && out, "jh_chain_create: null argument");
    JH_REQUIRE(type == JH_CHAIN_FORWARD || type == JH_CHAIN_ADJOINT || type == JH_CHAIN_NORMAL, "jh_chain_create: unknown chain type %d", type);
    JH_REQUIRE(!(type == JH_CHAIN_FORWARD && npost) && !(type == JH_CHAIN_ADJOINT && npre),
               "jh_chain_create: a FORWARD chain has no stages after A', an ADJOINT chain none before A");
    const bool grid = jhb::grid_chain_ok(op);
    if (!grid && (!(op->tall && op->uniform_rows && op->elementwise) || op->nrow < 2 || op->row_len[0] * (int64_t)jh_dtype_size(op->dtype) < 16))
        return jh_fail(JH_ERR_UNSUPPORTED, "jh_chain_create: needs a tall operator of >= 2 equal elementwise rows of at least 16 bytes, or an N x (2 .. 4) grid "
                                           "of equal diagonal / zero / identity / scalar blocks (knob grid_chain)");
    const size_t es = jh_dtype_size(op->dtype);
    const size_t sa = jh_dtype_complex(op->dtype) ? es / 2 : es;
    jh_chain *ch = new jh_chain();
    ch->ctx = op->ctx;
    ch->op = op;
    ch->type = type;
    ch->ncol = grid ? (int)op->ncol : 1;
    std::vector<const jh_chain_stage *> s_pre, s_mid, s_post;
    int st = build_prog("domain-side (before A)", npre, pre, op->dtype, 1, ch->args.pre, s_pre);
    if (st == JH_OK) st = build_prog("range-side", nmid, mid, op->dtype, op->nrow, ch->args.mid, s_mid);
    if (st == JH_OK) st = build_prog("domain-side (after A')", npost, post, op->dtype, 1, ch->args.post, s_post);
    if (st != JH_OK) { delete ch; return st; }
    bool scalar_aligned = true;
    auto note = [&](const void *p) {
        if (((uintptr_t)p) & 15u) ch->coeff16 = false;
        if (((uintptr_t)p) & (sa - 1)) scalar_aligned = false;
    };
    for (size_t q = 0; q < s_pre.size(); q++) { ch->args.pre_c[q] = s_pre[q]->coeff[0]; note(s_pre[q]->coeff[0]); }
    for (size_t q = 0; q < s_post.size(); q++) { ch->args.post_c[q] = s_post[q]->coeff[0]; note(s_post[q]->coeff[0]); }
    ch->nw = (int)s_mid.size();
    const size_t rw = (size_t)(ch->ncol + ch->nw);
    ch->host_tab.assign(rw * (size_t)op->nrow, 0);
    for (int w = 0; w < ch->nw; w++)
        for (int64_t i = 0; i < op->nrow; i++) {
            const void *p = s_mid[(size_t)w]->coeff[i];
            const uint64_t fl = s_mid[(size_t)w]->row_flags ? (s_mid[(size_t)w]->row_flags[i] & 3u) : 0u;
            note(p);
            if (((uint64_t)(uintptr_t)p) >> 48) scalar_aligned = false;           // (a device address above 2^48 does not exist on this platform)
            ch->host_tab[(size_t)i * rw + (size_t)ch->ncol + (size_t)w] = (uint64_t)(uintptr_t)p | (fl << 48);
        }
    if (!scalar_aligned) { delete ch; return jh_fail(JH_ERR_UNSUPPORTED, "jh_chain_create: a coefficient array is not aligned like its scalar"); }
    hipError_t e = jh_device_malloc(jh_ctx().device, (void **)&ch->dev_tab, ch->host_tab.size() * sizeof(uint64_t));
    if (e != hipSuccess) {
        delete ch;
        return jh_fail(e == hipErrorOutOfMemory ? JH_ERR_NOMEM : JH_ERR_HIP, "jh_chain_create: %s", hipGetErrorString(e));
    }
    ch->args.rows = ch->dev_tab;
    {
        const int st2 = chain_sync_rows(ch);
        if (st2 != JH_OK) { (void)hipFree(ch->dev_tab); delete ch; return st2; }
    }
    ch->stream_bytes = (double)op->nrow * (double)op->row_len[0] * (double)es * (double)(ch->ncol + ch->nw);
    if (type == JH_CHAIN_FORWARD) derive_progs(ch);
    if (ch->ncol > 1) {
        const ChainProg mids[3] = {ch->args.mid, ch->adj_args.mid, ch->nrm_args.mid};
        hipError_t e2 = jh_device_malloc(jh_ctx().device, (void **)&ch->dev_mid, sizeof(mids));
        if (e2 == hipSuccess) e2 = hipMemcpyAsync(ch->dev_mid, mids, sizeof(mids), hipMemcpyHostToDevice, jh_ctx().stream);
        if (e2 == hipSuccess) e2 = hipStreamSynchronize(jh_ctx().stream);
        if (e2 != hipSuccess) {
            if (ch->dev_mid) (void)hipFree(ch->dev_mid);
            (void)hipFree(ch->dev_tab);
            delete ch;
            return jh_fail(e2 == hipErrorOutOfMemory ? JH_ERR_NOMEM : JH_ERR_HIP, "jh_chain_create: %s", hipGetErrorString(e2));
        }
    }
    jh_handle_born(ch->ctx);
    *out = ch;
    return JH_OK;
}

int jh_chain_destroy(jh_chain *ch)
{
    if (!ch) return JH_OK;
    jh_quiesce_scope quiet(ch->ctx);
    if (ch->dev_tab) (void)hipFree(ch->dev_tab);
    if (ch->dev_mid) (void)hipFree(ch->dev_mid);
    jh_handle_died(ch->ctx);
    delete ch;
    return JH_OK;
}

int jh_chain_apply(const jh_chain *ch, jh_bvec *out, const jh_bvec *x, int accumulate)
{
    JH_REQUIRE(ch && out && x, "jh_chain_apply: null argument");
    const jh_blockop *op = ch->op;
    JH_TRY(jh_enter(op, out, x));
    JH_TRY(chain_check(ch, out, x, accumulate, "jh_chain_apply"));
    if (ch->op_gen != op->table_gen) JH_TRY(chain_sync_rows(const_cast<jh_chain *>(ch)));   // (the operator was pointed again: its SQUARE rows' arrays moved)
    if (ch->ncol > 1) return jhb::grid_chain_launch(ch, 0, ch->type, out->data, x->data, accumulate);
    const int64_t n = op->row_len[0];
    if (ch->type == JH_CHAIN_ADJOINT) return jhb::chain_launch_adjoint(ch, out->data, x->data, accumulate, 0, out->length);
    if (ch->type == JH_CHAIN_NORMAL) return jhb::chain_launch_normal(ch, out->data, x->data, accumulate, 0, out->length);
    return jh_by_dtype(op->dtype, "jh_chain_apply", [&](auto t) {
        using T = decltype(t);
        return launch_chain_fwd<typename T::S, T::E, T::NS>(ch, out->data, x->data, n * T::E, accumulate);
    });
}

// The ADJOINT / NORMAL chain over the domain's elements [first_elem, first_elem + count): what a host pipelining the exchange of the domain vector range
// by range against the kernels runs (weighted normal equations over a row partition, src/Jets.jl:530-540 over 1034-1057 summed across the ranks).  Writes
// out[first_elem, first_elem + count) and nothing else: each domain element depends on the same element of x (NORMAL) or of every row of x (ADJOINT).
int jh_chain_apply_range(const jh_chain *ch, jh_bvec *out, const jh_bvec *x, int accumulate, int64_t first_elem, int64_t count)
{
    JH_REQUIRE(ch && out && x, "jh_chain_apply_range: null argument");
    const jh_blockop *op = ch->op;
    JH_TRY(jh_enter(op, out, x));
    if (ch->type == JH_CHAIN_FORWARD)
        return jh_fail(JH_ERR_UNSUPPORTED, "jh_chain_apply_range: a FORWARD chain needs no exchange (each rank's rows depend on the replicated domain vector alone)");
    // a chain through an N x (2 .. 4) grid (knob grid_chain_range = 1): the range is positions INSIDE a block -- a grid kernel's lane owns one pack position
    // across all K columns --, the K pieces out_k[first_elem, first_elem + count) are written (k_grid_chain over those lanes, jh_grid_chain_kernels.h)
    const bool grid = ch->ncol > 1;
    if (grid && jh_ctx().grid_chain_range != 1)
        return jh_fail(JH_ERR_UNSUPPORTED, "jh_chain_apply_range: a grid chain has no ranged form (apply the whole vector)");
    JH_TRY(chain_check(ch, out, x, accumulate, "jh_chain_apply_range"));
    if (grid) {
        JH_TRY(jhb::grid_range_bounds(op, first_elem, count, "jh_chain_apply_range"));
        if (ch->op_gen != op->table_gen && jhb::stream_is_capturing(jh_ctx().stream))
            return jh_fail(JH_ERR_UNSUPPORTED, "jh_chain_apply_range: the operator was pointed again since the chain's row table was built, and the stream is capturing");
        if (count == 0) return JH_OK;
        if (ch->op_gen != op->table_gen) JH_TRY(chain_sync_rows(const_cast<jh_chain *>(ch)));
        return jhb::grid_chain_launch_range(ch, out->data, x->data, accumulate, first_elem, count);
    }
    JH_REQUIRE(first_elem >= 0 && count >= 0 && first_elem <= out->length - count,
               "jh_chain_apply_range: elements [%lld, %lld) outside the domain vector (%lld elements)", (long long)first_elem,
               (long long)(first_elem + count), (long long)out->length);
    const int64_t es = (int64_t)jh_dtype_size(op->dtype);
    JH_REQUIRE((first_elem * es) % 16 == 0 && ((count * es) % 16 == 0 || first_elem + count == out->length),
               "jh_chain_apply_range: range boundaries must be 16-byte aligned (the last range may end with the vector)");
    if (count == 0) return JH_OK;
    if (ch->op_gen != op->table_gen) {
        // the row table is copied to the device and the stream synchronised: not inside a capture (the whole-vector call keeps doing it)
        if (jhb::stream_is_capturing(jh_ctx().stream))
            return jh_fail(JH_ERR_UNSUPPORTED, "jh_chain_apply_range: the operator was pointed again since the chain's row table was built, and the stream is capturing");
        JH_TRY(chain_sync_rows(const_cast<jh_chain *>(ch)));
    }
    if (ch->type == JH_CHAIN_ADJOINT) return jhb::chain_launch_adjoint(ch, out->data, x->data, accumulate, first_elem, first_elem + count);
    return jhb::chain_launch_normal(ch, out->data, x->data, accumulate, first_elem, first_elem + count);
}

// the checks of the step and of the derived applications of a FORWARD chain: handle type, the operator's point, the row table (refreshed when the operator
// was pointed again -- declined while the stream is capturing: the copy to the device would be captured)
static int fwd_ready(const jh_chain *ch, const char *fn)
{
    JH_REQUIRE(ch->type == JH_CHAIN_FORWARD, "%s: needs a FORWARD chain (got type %d)", fn, ch->type);
    const jh_blockop *op = ch->op;
    if (op->nonlinear && !op->pointed)
        return jh_fail(JH_ERR_STATE, "%s: operator has nonlinear blocks and no linearisation point (jh_blockop_point)", fn);
    if (ch->op_gen != op->table_gen) {
        if (jhb::stream_is_capturing(jh_ctx().stream))
            return jh_fail(JH_ERR_UNSUPPORTED, "%s: the operator was pointed again since the chain's row table was built, and the stream is capturing", fn);
        JH_TRY(chain_sync_rows(const_cast<jh_chain *>(ch)));
    }
    return JH_OK;
}

// u <- alpha L v + beta u ;  w = L'u ;  ||u||^2 for L = R o A o P, in ONE pass (k_chain_adj MODE 2; through a grid, knob grid_chain_step = 1:
// k_grid_chain_step, jh_grid_chain_step.hip)
int jh_chain_bidiag_step(const jh_chain *fwd, jh_bvec *u, const jh_bvec *v, jh_bvec *w, double alpha, double beta, double *normsq)
{
    JH_REQUIRE(fwd && u && v && w, "jh_chain_bidiag_step: null argument");
    JH_REQUIRE(fwd->type == JH_CHAIN_FORWARD, "jh_chain_bidiag_step: needs a FORWARD chain (got type %d)", fwd->type);
    const jh_blockop *op = fwd->op;
    JH_TRY(jh_enter(op, u, v, w));
    const bool grid = fwd->ncol > 1;
    if (grid && jh_ctx().grid_chain_step == 0)
        return jh_fail(JH_ERR_UNSUPPORTED, "jh_chain_bidiag_step: a grid chain's one-pass step is off (knob grid_chain_step; run the FORWARD chain, then the ADJOINT)");
    if (!fwd->nrm_ok)
        return jh_fail(JH_ERR_UNSUPPORTED, "jh_chain_bidiag_step: R and R^H need more than %d range-side stages", JH_CHAIN_MAX_STAGES);
    const int64_t nrange = op->row_off[(size_t)op->nrow], ndom = op->col_off[(size_t)op->ncol];
    JH_REQUIRE(u->dtype == op->dtype && v->dtype == op->dtype && w->dtype == op->dtype, "jh_chain_bidiag_step: dtype mismatch");
    JH_REQUIRE(u->length == nrange && v->length == ndom && w->length == ndom, "jh_chain_bidiag_step: u must be a range vector, v and w domain vectors of the operator");
    JH_REQUIRE(w->data != v->data && u->data != v->data && u->data != w->data, "jh_chain_bidiag_step: u, v and w must be three vectors");
    if (!chain_vectors_ok(fwd, u->data, v->data) || !chain_vectors_ok(fwd, nullptr, w->data))
        return jh_fail(JH_ERR_UNSUPPORTED, "jh_chain_bidiag_step: a vector or coefficient array is not aligned like its scalar");
    JH_TRY(fwd_ready(fwd, "jh_chain_bidiag_step"));
    if (grid) return jhb::grid_chain_step(fwd, u->data, v->data, w->data, alpha, beta, normsq);
    return jhb::chain_launch_step(fwd, fwd->step_args, u->data, v->data, w->data, alpha, beta, normsq, 0, w->length, false);
}

// The step over the domain's elements [first_elem, first_elem + count): those columns of every row of u, that range of w, that range's share of ||u||^2
// -- what a host pipelining the exchange of w range by range against the kernels runs (weighted LSQR / CGLS over a row partition: src/Jets.jl:530-540
// over 1034-1057 summed across the ranks, the solvers over vec(L) 1138-1154).  The checks of jh_chain_bidiag_step and the bounds of
// jh_chain_apply_range, all before anything is touched.
int jh_chain_bidiag_step_range(const jh_chain *fwd, jh_bvec *u, const jh_bvec *v, jh_bvec *w, double alpha, double beta, int64_t first_elem, int64_t count,
                               double *normsq)
{
    JH_REQUIRE(fwd && u && v && w, "jh_chain_bidiag_step_range: null argument");
    JH_REQUIRE(fwd->type == JH_CHAIN_FORWARD, "jh_chain_bidiag_step_range: needs a FORWARD chain (got type %d)", fwd->type);
    const jh_blockop *op = fwd->op;
    JH_TRY(jh_enter(op, u, v, w));
    // (the handles' context is entered BEFORE the grid and nrm_ok refusals, which it used to follow: the knobs are per context and must be read in the
    // handle's.  A call whose handles live in different contexts therefore reports that, where it used to report the grid refusal first.)
    // a chain through an N x (2 .. 4) grid: knob grid_chain_range = 1, and grid_chain_step = 1 as for the whole-vector step (the rule of the bare grids'
    // ranged calls: a whole-vector knob also governs the ranged form); the range is positions INSIDE a block (k_grid_chain_step over those lanes)
    const bool grid = fwd->ncol > 1;
    if (grid && !(jh_ctx().grid_chain_range == 1 && jh_ctx().grid_chain_step == 1))
        return jh_fail(JH_ERR_UNSUPPORTED, "jh_chain_bidiag_step_range: a grid chain has no one-pass step (run the FORWARD chain, then the ADJOINT)");
    if (!fwd->nrm_ok)
        return jh_fail(JH_ERR_UNSUPPORTED, "jh_chain_bidiag_step_range: R and R^H need more than %d range-side stages", JH_CHAIN_MAX_STAGES);
    const int64_t nrange = op->row_off[(size_t)op->nrow], ndom = op->col_off[(size_t)op->ncol];
    JH_REQUIRE(u->dtype == op->dtype && v->dtype == op->dtype && w->dtype == op->dtype, "jh_chain_bidiag_step_range: dtype mismatch");
    JH_REQUIRE(u->length == nrange && v->length == ndom && w->length == ndom,
               "jh_chain_bidiag_step_range: u must be a range vector, v and w domain vectors of the operator");
    JH_REQUIRE(w->data != v->data && u->data != v->data && u->data != w->data, "jh_chain_bidiag_step_range: u, v and w must be three vectors");
    if (grid) {
        JH_TRY(jhb::grid_range_bounds(op, first_elem, count, "jh_chain_bidiag_step_range"));
        if (!chain_vectors_ok(fwd, u->data, v->data) || !chain_vectors_ok(fwd, nullptr, w->data))
            return jh_fail(JH_ERR_UNSUPPORTED, "jh_chain_bidiag_step_range: a vector or coefficient array is not aligned like its scalar");
        if (count == 0) {                                       // (nothing to do -- but the refusals of fwd_ready still come first)
            if (op->nonlinear && !op->pointed)
                return jh_fail(JH_ERR_STATE, "jh_chain_bidiag_step_range: operator has nonlinear blocks and no linearisation point (jh_blockop_point)");
            if (fwd->op_gen != op->table_gen && jhb::stream_is_capturing(jh_ctx().stream))
                return jh_fail(JH_ERR_UNSUPPORTED, "jh_chain_bidiag_step_range: the operator was pointed again since the chain's row table was built, and the stream is capturing");
            return JH_OK;
        }
        JH_TRY(fwd_ready(fwd, "jh_chain_bidiag_step_range"));
        return jhb::grid_chain_step_range(fwd, u->data, v->data, w->data, alpha, beta, first_elem, count, normsq);
    }
    JH_REQUIRE(first_elem >= 0 && count >= 0 && first_elem <= ndom - count,
               "jh_chain_bidiag_step_range: elements [%lld, %lld) outside the domain vector (%lld elements)", (long long)first_elem,
               (long long)(first_elem + count), (long long)ndom);
    const int64_t es = (int64_t)jh_dtype_size(op->dtype);
    JH_REQUIRE((first_elem * es) % 16 == 0 && ((count * es) % 16 == 0 || first_elem + count == ndom),
               "jh_chain_bidiag_step_range: range boundaries must be 16-byte aligned (the last range may end with the vector)");
    if (!jhb::tall_unaligned_ok(op, u->data, v->data) || !jhb::tall_unaligned_ok(op, nullptr, w->data))
        return jh_fail(JH_ERR_UNSUPPORTED, "jh_chain_bidiag_step_range: a vector or coefficient array is not aligned like its scalar");
    if (count == 0) return JH_OK;
    JH_TRY(fwd_ready(fwd, "jh_chain_bidiag_step_range"));
    return jhb::chain_launch_step(fwd, fwd->step_args, u->data, v->data, w->data, alpha, beta, normsq, first_elem, first_elem + count, true);
}

}  // extern "C"

namespace jhb {
// L' (which == JH_CHAIN_ADJOINT: out = L' in, in a range vector) or L'L (JH_CHAIN_NORMAL) of a FORWARD chain, through the derived programs: the solver
// loops of jh_lsqr.hip on a chain
int chain_apply_derived(const jh_chain *fwd, int which, jh_bvec *out, const jh_bvec *in)
{
    JH_REQUIRE(fwd && out && in, "chain_apply_derived: null argument");
    const jh_blockop *op = fwd->op;
    JH_TRY(jh_enter(op, out, in));
    JH_TRY(fwd_ready(fwd, "chain_apply_derived"));
    if (which == JH_CHAIN_NORMAL && !fwd->nrm_ok)
        return jh_fail(JH_ERR_UNSUPPORTED, "chain_apply_derived: R and R^H need more than %d range-side stages", JH_CHAIN_MAX_STAGES);
    const int64_t nrange = op->row_off[(size_t)op->nrow], ndom = op->col_off[(size_t)op->ncol];
    JH_REQUIRE(out->dtype == op->dtype && in->dtype == op->dtype && out->data != in->data, "chain_apply_derived: dtype mismatch or aliasing");
    JH_REQUIRE(out->length == ndom && in->length == (which == JH_CHAIN_ADJOINT ? nrange : ndom), "chain_apply_derived: vector lengths");
    const bool ok = which == JH_CHAIN_ADJOINT ? chain_vectors_ok(fwd, in->data, out->data)
                                              : chain_vectors_ok(fwd, nullptr, out->data) && chain_vectors_ok(fwd, nullptr, in->data);
    if (!ok) return jh_fail(JH_ERR_UNSUPPORTED, "chain_apply_derived: a vector is not aligned like its scalar");
    if (fwd->ncol > 1) return grid_chain_launch(fwd, which == JH_CHAIN_ADJOINT ? 1 : 2, which, out->data, in->data, 0);
    if (which == JH_CHAIN_ADJOINT) return chain_launch_adjoint(fwd, out->data, in->data, 0, 0, out->length, &fwd->adj_args);
    return chain_launch_normal(fwd, out->data, in->data, 0, 0, out->length, &fwd->nrm_args);
}
}  // namespace jhb

namespace jhb {
// may the solver loops run on this chain (jh_*_solve_chain)?  The checks of jh_chain_bidiag_step on the solver's vectors, before anything is touched
int chain_solver_ok(const jh_chain *fwd, const jh_bvec *u, const jh_bvec *x, const jh_blockop **op, bool needs_step)
{
    JH_REQUIRE(fwd->type == JH_CHAIN_FORWARD, "jh_*_solve_chain: needs a FORWARD chain (got type %d)", fwd->type);
    const jh_context *cx = jh_ctx_by_id(fwd->ctx);                              // (the handle's context: the caller enters it after these checks)
    if (needs_step && fwd->ncol > 1 && !(cx && cx->grid_chain_step == 1))
        return jh_fail(JH_ERR_UNSUPPORTED, "jh_*_solve_chain: a grid chain's one-pass step is off (knob grid_chain_step: LSQR / CGLS keep their two-pass loops; CGNR runs)");
    if (!fwd->nrm_ok)
        return jh_fail(JH_ERR_UNSUPPORTED, "jh_*_solve_chain: R and R^H need more than %d range-side stages", JH_CHAIN_MAX_STAGES);
    const jh_blockop *o = fwd->op;
    const int64_t nrange = o->row_off[(size_t)o->nrow], ndom = o->col_off[(size_t)o->ncol];
    JH_REQUIRE(u->dtype == o->dtype && x->dtype == o->dtype && u->length == nrange && x->length == ndom,
               "jh_*_solve_chain: the right-hand side must be a range vector and x a domain vector of the chain's operator");
    if (!chain_vectors_ok(fwd, u->data, x->data))
        return jh_fail(JH_ERR_UNSUPPORTED, "jh_*_solve_chain: a vector is not aligned like its scalar");
    *op = o;
    return JH_OK;
}
}  // namespace jhb

// ---- the chain kernels as the library's own adjoint / fused A'A of operators with rows of several kinds (round 6) -----------------------------------
// With EMPTY stage lists the ADJOINT chain is m = sum_i conj(a_i) .* d_i -- jh_blockop_mul_adj --, the NORMAL chain jh_blockop_normal_mul, over packed 8-byte row records requested a batch ahead,
// where k_tall_diag_adj<MIXED> reads a 48-byte block descriptor per row behind a kind switch.  On rows of up to ~2 MiB (one workgroup per CU or the split
// walk) that is the difference: same box, one identity row among the diagonals, TB/s library | chain kernel: 256 x 2 MiB 5.4-5.8 | 6.2-6.85,
// 4096 x 1 MiB 5.35-5.64 | 6.8-7.0, 2048 x 512 KiB 5.3-6.1 | 6.1-6.6, 262144 x 513 elements (off the grid) 4.4 | 5.5; from 4 MiB rows on they are
// level and the fat shapes of k_tall_diag_adj win (tools/exp_chain_vs_mixed.py, profiles/exp_r06_chain_vs_mixed.txt).  Later in the round both kernels learnt to run a
// batch of PLAIN diagonals through the all-diagonal kernel's tight loop (the per-row kind switch was the cost): the adjoints drew level, and the fused A'A of the chain
// kernel pulled ahead -- one identity row: 256 x 2 MiB 5.2 | 6.6-6.7, 1024 x 1 MiB 5.8 | 6.7-7.0, 1024 x 4 MiB 6.2 | 6.95 -- so rows of up to 4 MiB take it for both.  Same bits (rows in order from +0);
// where the rows are summed in parts the part count may differ from k_tall_diag_adj's (tolerance parity either way).
namespace jhb {
int bare_chain(const jh_blockop *op, void *out, const void *in, int mode, bool *took)
{
    *took = false;
    jh_context &c = jh_ctx();
    const int64_t row_bytes = op->row_len[0] * (int64_t)jh_dtype_size(op->dtype);
    if (!c.adj_bare_chain || op->nrow < 2 || row_bytes < 16 || row_bytes > ((int64_t)4 << 20)) return JH_OK;
    if (c.adj_rows_per_launch != 0 || (mode == 0 && (c.adj_from_found || c.adj_in_scale != 1.0))) return JH_OK;
    const char *sb = (const char *)c.scratch_dev;
    if (sb && (const char *)out >= sb && (const char *)out < sb + c.scratch_cap) return JH_OK;   // an output reserved behind split_adjoint_tmp's slabs: that route's part count
    jh_chain *&slot = op->bare_chain[mode ? 1 : 0];
    if (!slot || slot->op_gen != op->table_gen) {
        if (stream_is_capturing(c.stream)) return JH_OK;                                          // (building or refreshing the row table copies to the device)
        if (!slot) {
            jh_chain *ch = nullptr;
            const int st = jh_chain_create(op, mode ? JH_CHAIN_NORMAL : JH_CHAIN_ADJOINT, 0, nullptr, 0, nullptr, 0, nullptr, &ch);
            if (st == JH_ERR_UNSUPPORTED) return JH_OK;
            JH_TRY(st);
            slot = ch;
        } else {
            JH_TRY(chain_sync_rows(slot));
        }
    }
    *took = true;
    const int64_t ndom = op->col_off[(size_t)op->ncol];
    return mode ? chain_launch_normal(slot, out, in, 0, 0, ndom) : chain_launch_adjoint(slot, out, in, 0, 0, ndom);
}
}  // namespace jhb
