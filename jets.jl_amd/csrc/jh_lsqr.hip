// jh_lsqr.hip -- LSQR (Paige & Saunders, ACM TOMS 8(1), 1982) over a tall all-DIAG block operator, entirely behind the C
// ABI: the caller of the block mul! path that BASELINE.json configs[4] names.  The reference reaches it as
// `lsqr(vec(A), vec(d))` of IterativeSolvers.jl (src/Jets.jl:1143-1152, docs/src/index.md:235-246), an un-vendored
// package, so this is the published algorithm written from scratch -- the same recurrences as jets.jl_amd/lsqr.py, which
// stays the driver for arbitrary operators; results are checked against the fp64 CPU LSQR of oracle/lsqr_ref.py.
//
// One iteration = ONE pass over the operator and the range vector (jh_blockop_bidiag_step: u <- A v - (alpha/beta) u,
// ||u||^2 and A'u together), then domain-sized updates.  u is never normalised in memory: it holds beta*u and the scale is
// carried into the next step.  With jh_comm_init_rank done (one process per GPU, this rank holding its block rows) the local
// A'u is all-reduced with RCCL and ||u||^2 with a scalar all-reduce: row-partitioned LSQR without a line of host code.
#include "jh_internal.h"

#include <cmath>

namespace {

// ---- the domain-side half of an iteration in two kernels (instead of five broadcasts and two norms) ----------------
// All coefficients are real, so a complex vector is 2n reals here.  Rounding sequence of every element == the broadcasts
// they replace (jh_lincomb: every product rounded, then the sum); the norms are summed in another (fixed) order than
// jh_norm's, so alpha agrees with the unfused loop to fp64 round-off, not to the bit.
template <int BLK> __device__ inline void wg_sum_to(double v, double *slot)
{
    __shared__ double sm[BLK / 64];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        double r = sm[0];
#pragma unroll
        for (int w = 1; w < BLK / 64; w++) r += sm[w];
        *slot = r;
    }
}

// v <- c0*atu + c1*v ; partial ||v||^2
template <typename S>
__global__ __launch_bounds__(256) void k_lsqr_vhat(S *v, const S *__restrict__ atu, int64_t n, S c0, S c1, double *__restrict__ partials)
{
    double nrm = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const S a = c0 * atu[i], b = c1 * v[i];
        const S r = a + b;
        v[i] = r;
        nrm += (double)r * (double)r;
    }
    wg_sum_to<256>(nrm, partials + blockIdx.x);
}

// v <- cv*v (normalise) ; x <- x + t1*w ; w <- v + t2*w ; partial ||w_new||^2
template <typename S>
__global__ __launch_bounds__(256) void k_lsqr_xw(S *v, S *x, S *w, int64_t n, S cv, S t1, S t2, double *__restrict__ partials)
{
    double nrm = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const S vn = cv * v[i];
        const S wo = w[i];
        const S xa = (S)1 * x[i], xb = t1 * wo;
        const S wa = (S)1 * vn, wb = t2 * wo;
        const S wn = wa + wb;
        v[i] = vn;
        x[i] = xa + xb;
        w[i] = wn;
        nrm += (double)wn * (double)wn;
    }
    wg_sum_to<256>(nrm, partials + blockIdx.x);
}

// one workgroup folds the per-workgroup partials in index order (deterministic)
__global__ __launch_bounds__(256) void k_lsqr_fold(const double *__restrict__ partials, int nparts, double *__restrict__ out)
{
    double v = 0.0;
    for (int i = threadIdx.x; i < nparts; i += 256) v += partials[i];
    wg_sum_to<256>(v, out);
}

// one member's domain-sized work vectors (and, LSQR: its per-workgroup partials), made in the member's context and released on every exit path
template <int N> struct DomVecs {
    jh_bvec *vec[N] = {};
    double *parts = nullptr;
    DomVecs() = default;
    DomVecs(const DomVecs &) = delete;
    DomVecs &operator=(const DomVecs &) = delete;
    ~DomVecs()
    {
        if (parts) (void)hipFree(parts);
        for (jh_bvec *p : vec)
            if (p) (void)jh_bvec_destroy(p);
    }
    jh_bvec *operator[](int i) const { return vec[i]; }
    int create(int64_t n, int dtype, size_t nparts = 0)
    {
        const int64_t len1[1] = {n};
        for (jh_bvec *&p : vec) JH_TRY(jh_bvec_create(1, len1, dtype, &p));
        if (nparts) JH_CHECK_HIP(jh_device_malloc(jh_ctx().device, (void **)&parts, sizeof(double) * nparts));
        return JH_OK;
    }
};
enum { V, W, ATU };                              // LSQR's three
enum { P, S, Y };                                // CGLS's and CGNR's

int lincomb1(jh_bvec *dst, double c0, const jh_bvec *x0)
{
    const double coef[2] = {c0, 0.0};
    const jh_bvec *xs[1] = {x0};
    return jh_lincomb(dst, 1, coef, xs);
}

int lincomb2(jh_bvec *dst, double c0, const jh_bvec *x0, double c1, const jh_bvec *x1)
{
    const double coef[4] = {c0, 0.0, c1, 0.0};
    const jh_bvec *v[2] = {x0, x1};
    return jh_lincomb(dst, 2, coef, v);
}

// workgroups of the domain-side kernels: a complex vector is 2n reals for these real-coefficient updates
int dom_grid(int64_t n, int dtype)
{
    const int64_t ns_dom = n * (jh_dtype_complex(dtype) ? 2 : 1);
    const int grid = (int)((ns_dom + 255) / 256 < 4096 ? (ns_dom + 255) / 256 : 4096);
    return grid < 1 ? 1 : grid;
}

int launch_vhat(int dtype, jh_bvec *v, const jh_bvec *atu, double c0, double c1, double *parts, int grid)
{
    return jh_by_dtype(dtype, "lsqr v update", [&](auto t) -> int {
        using T = typename decltype(t)::S;
        hipLaunchKernelGGL((k_lsqr_vhat<T>), dim3(grid), dim3(256), 0, jh_ctx().stream, (T *)v->data, (const T *)atu->data, v->length * decltype(t)::E, (T)c0, (T)c1, parts);
        JH_CHECK_HIP(hipGetLastError());
        return JH_OK;
    });
}

int launch_xw(int dtype, jh_bvec *v, jh_bvec *x, jh_bvec *w, double cv, double t1, double t2, double *parts, int grid)
{
    return jh_by_dtype(dtype, "lsqr x/w update", [&](auto t) -> int {
        using T = typename decltype(t)::S;
        hipLaunchKernelGGL((k_lsqr_xw<T>), dim3(grid), dim3(256), 0, jh_ctx().stream, (T *)v->data, (T *)x->data, (T *)w->data, v->length * decltype(t)::E, (T)cv, (T)t1, (T)t2, parts);
        JH_CHECK_HIP(hipGetLastError());
        return JH_OK;
    });
}

}  // namespace

// ---- small operators: the recurrences live on the DEVICE and one iteration is a hipGraph -------------------------------------
// The loop below (lsqr_impl) synchronises the host twice per iteration to turn two sums into the next coefficients.  For an
// operator whose pass takes a few hundred microseconds that costs as much as the kernels (64 x 64^3: 84 us per iteration, 35 of
// them on the device).  Here the scalars of Paige & Saunders' recurrences are a struct in device memory, two one-thread kernels
// update it from the sums with the two functions the host loop calls (lsqr_s1, lsqr_s2: the recurrences exist once), the step / v / x-w kernels read
// their coefficients from it, and a finished solve turns every kernel into a no-op -- so an iteration has fixed launch parameters,
// is captured ONCE as a hipGraph and replayed; the host looks at the `done` flag every few iterations.  Same kernels, same
// arithmetic: the iterates are those of lsqr_impl bit for bit.
struct LsqrDev {
    double alpha, beta, rhobar, phibar, anorm, ddnorm, res2, xxnorm, z, cs2, sn2, bnorm, wnorm, damp, atol, btol, ctol;
    double r1norm, r2norm, acond, arnorm, xnorm;
    double coef_step[2];                         // (1, -alpha / beta): the next one-pass step
    double coef_vhat[2];                         // (1 / beta, -beta)
    double coef_xw[3];                           // (cv, t1, t2)
    int itn, istop, done, pending, skipv, maxiter, force, halt;   // halt = done || pending: the NEXT step is not to run (five-node iteration below)
};

// after the step: beta from ||u||^2, ||w|| of the previous iteration, the coefficients of the v update
__host__ __device__ inline void lsqr_s1(LsqrDev *st, double normsq, const double *__restrict__ slot_w)
{
    st->itn++;
    st->beta = sqrt(normsq);
    if (st->itn >= 2) st->wnorm = sqrt(*slot_w);
    st->skipv = 1;
    if (st->beta > 0) {
        st->anorm = sqrt(st->anorm * st->anorm + st->alpha * st->alpha + st->beta * st->beta + st->damp * st->damp);
        st->coef_vhat[0] = 1.0 / st->beta;
        st->coef_vhat[1] = -st->beta;
        st->skipv = 0;
    }
}

// after the v update: alpha, the rotations, the coefficients of the x / w update, the norm estimates, the stopping rules
__host__ __device__ inline void lsqr_s2(LsqrDev *st, double sum_v, double *__restrict__ history)
{
    double alpha = st->alpha, beta = st->beta, rhobar = st->rhobar, phibar = st->phibar;
    double cv = 1.0;
    if (!st->skipv) {
        alpha = sqrt(sum_v);
        if (alpha > 0) cv = 1.0 / alpha;
    }
    const double damp = st->damp;
    const double rhobar1 = sqrt(rhobar * rhobar + damp * damp);
    const double rho = sqrt(rhobar1 * rhobar1 + beta * beta);
    if (!(rhobar1 > 0 && std::isfinite(rho))) {  // far past convergence under force_maxiter: the recurrences have underflowed
        if (!st->istop) st->istop = 6;
        st->itn--;
        st->alpha = alpha;
        st->done = 1;
        st->halt = 1;
        return;
    }
    const double cs1 = rhobar / rhobar1, sn1 = damp / rhobar1;
    const double psi = sn1 * phibar;
    phibar = cs1 * phibar;
    const double cs = rhobar1 / rho, sn = beta / rho;
    const double theta = sn * alpha;
    rhobar = -cs * alpha;
    const double phi = cs * phibar;
    phibar = sn * phibar;
    const double tau = sn * phi;
    const double t1 = phi / rho, t2 = -theta / rho;
    st->ddnorm += (st->wnorm / rho) * (st->wnorm / rho);
    st->coef_xw[0] = cv;
    st->coef_xw[1] = t1;
    st->coef_xw[2] = t2;
    const double delta = st->sn2 * rho, gambar = -st->cs2 * rho, rhs = phi - delta * st->z, zbar = rhs / gambar;
    const double xnorm = sqrt(st->xxnorm + zbar * zbar);
    const double gamma = sqrt(gambar * gambar + theta * theta);
    st->cs2 = gambar / gamma;
    st->sn2 = theta / gamma;
    st->z = rhs / gamma;
    st->xxnorm += st->z * st->z;
    const double anorm = st->anorm;
    const double acond = anorm * sqrt(st->ddnorm);
    const double res1 = phibar * phibar;
    st->res2 += psi * psi;
    const double rnorm = sqrt(res1 + st->res2);
    const double arnorm = alpha * fabs(tau);
    const double r1sq = rnorm * rnorm - damp * damp * st->xxnorm;
    const double r1norm = sqrt(fabs(r1sq)) * (r1sq >= 0 ? 1.0 : -1.0);
    const int itn = st->itn;
    if (history) { history[2 * (itn - 1)] = r1norm; history[2 * (itn - 1) + 1] = arnorm; }
    const double eps = 2.220446049250313e-16, bnorm = st->bnorm;
    const double test1 = bnorm > 0 ? rnorm / bnorm : 0.0;
    const double test2 = rnorm > 0 ? arnorm / (anorm * rnorm + eps) : 0.0;
    const double test3 = 1.0 / (acond + eps);
    const double t1_ = bnorm > 0 ? test1 / (1 + anorm * xnorm / bnorm) : 0.0;
    const double rtol = bnorm > 0 ? st->btol + st->atol * anorm * xnorm / bnorm : 0.0;
    int istop = st->istop;
    if (itn >= st->maxiter) istop = 7;
    if (1 + test3 <= 1) istop = 6;
    if (1 + test2 <= 1) istop = 5;
    if (1 + t1_ <= 1) istop = 4;
    if (test3 <= st->ctol) istop = 3;
    if (test2 <= st->atol) istop = 2;
    if (test1 <= rtol) istop = 1;
    st->istop = istop;
    st->alpha = alpha;
    st->rhobar = rhobar;
    st->phibar = phibar;
    st->r1norm = r1norm;
    st->r2norm = rnorm;
    st->acond = acond;
    st->arnorm = arnorm;
    st->xnorm = xnorm;
    st->coef_step[0] = 1.0;
    st->coef_step[1] = -alpha / beta;
    if (istop && !(st->force && itn < st->maxiter && alpha > 0 && beta > 0)) {
        st->pending = 1;                         // x and w of THIS iteration are still updated
        st->halt = 1;
    }
}

// the state before the first iteration, from the start-up's alpha = ||A'u|| / beta, beta = ||u||, ||b|| and ||w||
static LsqrDev lsqr_state_init(double alpha, double beta, double bnorm, double wnorm, double damp, double atol, double btol, double conlim, int maxiter,
                               int force_maxiter)
{
    LsqrDev h{};
    h.alpha = alpha;
    h.beta = beta;
    h.rhobar = alpha;
    h.phibar = beta;
    h.cs2 = -1.0;
    h.bnorm = bnorm;
    h.wnorm = wnorm;
    h.damp = damp;
    h.atol = atol;
    h.btol = btol;
    h.ctol = conlim > 0 ? 1.0 / conlim : 0.0;
    h.r1norm = h.r2norm = beta;
    h.arnorm = alpha * beta;
    h.coef_step[0] = 1.0;
    h.coef_step[1] = -alpha / beta;
    h.maxiter = maxiter;
    h.force = force_maxiter ? 1 : 0;
    return h;
}

static void lsqr_result_from(const LsqrDev &h, jh_lsqr_result *res)
{
    res->istop = h.istop;
    res->itn = h.itn;
    res->r1norm = h.r1norm;
    res->r2norm = h.r2norm;
    res->anorm = h.anorm;
    res->acond = h.acond;
    res->arnorm = h.arnorm;
    res->xnorm = h.xnorm;
}

__global__ void k_lsqr_s1(LsqrDev *st, const double *__restrict__ normsq, const double *__restrict__ slot_w)
{
    if (!st->done) lsqr_s1(st, *normsq, slot_w);
}
__global__ void k_lsqr_s2(LsqrDev *st, const double *__restrict__ slot_v, double *__restrict__ history)
{
    if (!st->done) lsqr_s2(st, *slot_v, history);
}
__global__ void k_lsqr_s3(LsqrDev *st)
{
    if (st->pending) st->done = 1;
}

// the same three steps FUSED into the single-workgroup folds that precede them (k_sum_partials / k_lsqr_fold: the same strided sums
// and the same tree, so the same bits): an iteration is then five graph nodes instead of ten, and the chain of dependent small
// kernels is what a small operator's iteration costs
template <int BLK> __device__ inline double wg_sum_value(double v)
{
    __shared__ double sm[BLK / 64];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = sm[0];
#pragma unroll
    for (int w = 1; w < BLK / 64; w++) r += sm[w];
    return r;                                    // (valid in every lane)
}
// (round 4: FIVE nodes.  The fold of ||w||^2 that closed an iteration only fed the NEXT iteration's first scalar step, and its
// "pending -> done" can wait until then as long as the step in between does not run: the step looks at `halt`, this fold finishes
// the solve and sums the x / w kernel's partials itself -- same strided sums, same tree, same bits as the separate fold.)
__global__ __launch_bounds__(256) void k_lsqr_fold_s1(const double *__restrict__ partials, int64_t nparts, LsqrDev *st, const double *__restrict__ parts_w, int nparts_w,
                                                      double *__restrict__ slot_w)
{
    if (st->done) return;
    if (st->pending) {
        if (threadIdx.x == 0) st->done = 1;
        return;
    }
    double w = 0.0;
    for (int i = threadIdx.x; i < nparts_w; i += 256) w += parts_w[i];
    const double rw = wg_sum_value<256>(w);
    __syncthreads();                             // (wg_sum_value's scratch is used again)
    double v = 0.0;
    for (int64_t i = threadIdx.x; i < nparts; i += 256) v += partials[i];
    const double r = wg_sum_value<256>(v);
    if (threadIdx.x == 0) {
        *slot_w = rw;
        lsqr_s1(st, 0.0 + r, slot_w);            // (k_sum_partials adds its sum to a zeroed accumulator)
    }
}
__global__ __launch_bounds__(256) void k_lsqr_fold_s2(const double *__restrict__ partials, int nparts, LsqrDev *st, double *__restrict__ history)
{
    if (st->done) return;
    double v = 0.0;
    for (int i = threadIdx.x; i < nparts; i += 256) v += partials[i];
    const double r = wg_sum_value<256>(v);
    if (threadIdx.x == 0) lsqr_s2(st, r, history);
}

template <typename S>
__global__ __launch_bounds__(256) void k_lsqr_vhat_dev(S *v, const S *__restrict__ atu, int64_t n, const LsqrDev *__restrict__ st, double *__restrict__ partials)
{
    if (st->done || st->skipv) return;
    const S c0 = (S)st->coef_vhat[0], c1 = (S)st->coef_vhat[1];
    double nrm = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const S a = c0 * atu[i], b = c1 * v[i];
        const S r = a + b;
        v[i] = r;
        nrm += (double)r * (double)r;
    }
    wg_sum_to<256>(nrm, partials + blockIdx.x);
}

template <typename S>
__global__ __launch_bounds__(256) void k_lsqr_xw_dev(S *v, S *x, S *w, int64_t n, const LsqrDev *__restrict__ st, double *__restrict__ partials)
{
    if (st->done) return;
    const S cv = (S)st->coef_xw[0], t1 = (S)st->coef_xw[1], t2 = (S)st->coef_xw[2];
    double nrm = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const S vn = cv * v[i];
        const S wo = w[i];
        const S xa = (S)1 * x[i], xb = t1 * wo;
        const S wa = (S)1 * vn, wb = t2 * wo;
        const S wn = wa + wb;
        v[i] = vn;
        x[i] = xa + xb;
        w[i] = wn;
        nrm += (double)wn * (double)wn;
    }
    wg_sum_to<256>(nrm, partials + blockIdx.x);
}

// the same two launches with the coefficients in device memory (no error check here: the iteration that enqueues them asks once)
static int launch_vhat_dev(int dtype, jh_bvec *v, const jh_bvec *atu, const LsqrDev *st, double *parts, int grid)
{
    return jh_by_dtype(dtype, "lsqr v update", [&](auto t) -> int {
        using T = typename decltype(t)::S;
        hipLaunchKernelGGL((k_lsqr_vhat_dev<T>), dim3(grid), dim3(256), 0, jh_ctx().stream, (T *)v->data, (const T *)atu->data, v->length * decltype(t)::E, st, parts);
        return JH_OK;
    });
}

static int launch_xw_dev(int dtype, jh_bvec *v, jh_bvec *x, jh_bvec *w, const LsqrDev *st, double *parts, int grid)
{
    return jh_by_dtype(dtype, "lsqr x/w update", [&](auto t) -> int {
        using T = typename decltype(t)::S;
        hipLaunchKernelGGL((k_lsqr_xw_dev<T>), dim3(grid), dim3(256), 0, jh_ctx().stream, (T *)v->data, (T *)x->data, (T *)w->data, v->length * decltype(t)::E, st, parts);
        return JH_OK;
    });
}

// WHO sums across shards of the operator:
//   none   one context holds all rows (jh_lsqr_solve);
//   ranks  op/u are THIS rank's block rows of a row-partitioned operator and the exchange runs over the communicator of
//          jh_comm_init_rank -- the CALLER says so (jh_lsqr_solve_partitioned); a communicator merely being alive never turns a
//          rank-local solve into a collective one;
//   team   this process holds M shards, one per member context of a single-process team (jh_comm_init_all): the members'
//          kernels are enqueued one after the other (they return after enqueue, so the GPUs run concurrently), the ranged
//          all-reduces of a range are issued as one group, scalars are added on the host from the members' partials, and the
//          domain-side updates run redundantly on every member with the SAME host scalars, so the replicas stay bit-identical.
enum class Exch { none, ranks, team };

// The four passes the loops below take from a shard: a block operator's fused kernels, or (one GPU, jh_*_solve_chain) a FORWARD chain L = R o A o P
// and the programs derived from it.  A chain has no forward-with-axpby of its own: the warm start u <- b - L x0 is one step into a scratch domain vector.
// An N x (2 .. 4) grid (one GPU, jh_lsqr_solve / jh_cgls_solve) has no forward-with-axpby either: its warm start is the same scratch step (jh_grid_step.hip).
struct Passes {
    const jh_blockop *op = nullptr;
    const jh_chain *ch = nullptr;
    bool grid = false;                           // op is a grid (jhb::grid_step_ok)
    jh_bvec *scratch = nullptr;                  // (chain, grid: the step's w of the warm start)
    Passes() = default;
    Passes(const Passes &) = delete;
    Passes &operator=(const Passes &) = delete;
    ~Passes() { if (scratch) (void)jh_bvec_destroy(scratch); }
    // u <- a*(L x) + b*u, ||u||^2
    int fwd_axpby(jh_bvec *u, const jh_bvec *x, double a, double b, double *normsq)
    {
        if (!ch && !grid) return jh_blockop_mul_axpby(op, u, x, a, b, normsq);
        if (!scratch) {
            const int64_t len1[1] = {x->length};
            JH_TRY(jh_bvec_create(1, len1, x->dtype, &scratch));
        }
        return ch ? jh_chain_bidiag_step(ch, u, x, scratch, a, b, normsq) : jh_blockop_bidiag_step(op, u, x, scratch, a, b, normsq);
    }
    // out = L' in
    int adjoint(jh_bvec *out, const jh_bvec *in) { return ch ? jhb::chain_apply_derived(ch, JH_CHAIN_ADJOINT, out, in) : jh_blockop_mul_adj(op, out, in); }
    // u <- a*(L v) + b*u ; w = L'u ; ||u||^2
    int step(jh_bvec *u, const jh_bvec *v, jh_bvec *w, double a, double b, double *normsq)
    {
        return ch ? jh_chain_bidiag_step(ch, u, v, w, a, b, normsq) : jh_blockop_bidiag_step(op, u, v, w, a, b, normsq);
    }
    // y = L'L m
    int normal(jh_bvec *y, const jh_bvec *m) { return ch ? jhb::chain_apply_derived(ch, JH_CHAIN_NORMAL, y, m) : jh_blockop_normal_mul(op, y, m); }
};

// One solve's shards -- member k's operator, its rows of the right-hand side and its replica of x -- and the steps the three loops below take over
// them.  `who` is the public name the messages carry.
struct Shards {
    const char *const who;
    const int M;
    const jh_blockop *const *const ops;
    jh_bvec *const *const rhs, *const *const xs;
    const Exch ex;
    int64_t n = 0, chunk = 0;                    // elements of x; of an exchange range: 4 ranges, on 64 KiB boundaries
    int dtype = 0;
    std::vector<double> locals;                  // one scalar per member (sum)
    Shards(const char *who_, int M_, const jh_blockop *const *ops_, jh_bvec *const *rhs_, jh_bvec *const *xs_, Exch ex_)
        : who(who_), M(M_), ops(ops_), rhs(rhs_), xs(xs_), ex(ex_) {}
    Shards(const Shards &) = delete;
    Shards &operator=(const Shards &) = delete;

    int use(int k) const { return jh_enter(ops[k], rhs[k], xs[k]); }
    // the common checks; takes(k) is the solver's own rule, asked member by member BEFORE anything is touched: the caller can still take another path
    template <class F> int init(const jh_lsqr_result *res, int maxiter, F &&takes, const char *needs)
    {
        JH_REQUIRE(ops && rhs && xs && res && M >= 1, "%s: null argument", who);
        JH_REQUIRE(maxiter >= 0, "%s: maxiter must be >= 0", who);
        for (int k = 0; k < M; k++) JH_REQUIRE(ops[k] && rhs[k] && xs[k], "%s: null argument (member %d)", who, k);
        JH_TRY(use(0));
        int64_t nb = 0;
        JH_TRY(jh_bvec_info(xs[0], &nb, &n, &dtype, nullptr));
        for (int k = 0; k < M; k++) {
            JH_REQUIRE(xs[k]->length == n && xs[k]->dtype == dtype, "%s: member %d's x differs in length or element type", who, k);
            if (!takes(k)) return jh_fail(JH_ERR_UNSUPPORTED, "%s: needs %s", who, needs);
        }
        chunk = ((n + 3) / 4 + 16383) / 16384 * 16384;
        locals.assign((size_t)M, 0.0);
        return JH_OK;
    }
    bool tall(int k) const { return jh_blockop_tall_step_ok(ops[k], rhs[k]->data, xs[k]->data); }   // (rows off the 16-byte pack grid too)
    // sum of one scalar per member, in index order, then over the ranks
    int sum(const std::vector<double> &vals, double *out) const
    {
        double s = 0.0;
        for (double v : vals) s += v;
        *out = s;
        if (ex == Exch::ranks) JH_TRY(jh_comm_allreduce_scalars(out, 1, 0));
        return JH_OK;
    }
    // the members' all-reduces of one collective: a team's as one group (the first error is kept, the group is closed all the same)
    template <class F> int grouped(F &&one) const
    {
        if (ex == Exch::none) return JH_OK;
        if (ex == Exch::team) { JH_TRY(use(0)); JH_TRY(jh_comm_group_begin()); }
        int st = JH_OK;
        for (int k = 0; k < M && st == JH_OK; k++) st = one(k);
        if (ex == Exch::team) { (void)use(0); const int st2 = jh_comm_group_end(); if (st == JH_OK) st = st2; }
        return st;
    }
    template <class F> int for_ranges(F &&f) const
    {
        for (int64_t lo = 0; lo < n; lo += chunk) JH_TRY(f(lo, lo + chunk < n ? chunk : n - lo));
        return JH_OK;
    }
    // The pipelined distributed step  rhs_k <- a*(A_k v) + b*rhs_k ; out = sum_k A_k' rhs_k ; ||rhs||^2:  every shard's rows in element ranges -- the
    // all-reduce of a finished range of `out` runs on the exchange stream while the kernel of the next range computes; the norm accumulates on the
    // device and is summed behind the last range: ONE host synchronisation per shard for the whole step (a team: member 0 last, whose
    // synchronisation also lands what its stream copied before)
    template <class FV, class FO> int ranged_step(FV &&v_of, FO &&out_of, double a, double b, double *normsq) const
    {
        for (int k = 0; k < M; k++) { JH_TRY(use(k)); JH_TRY(jh_normsq_reset()); }
        JH_TRY(for_ranges([&](int64_t lo, int64_t cnt) -> int {
            for (int k = 0; k < M; k++) JH_TRY(jh_blockop_bidiag_step_range(ops[k], rhs[k], v_of(k), out_of(k), a, b, lo, cnt, nullptr));
            return grouped([&](int k) { return jh_comm_allreduce_sum_range(out_of(k), lo, cnt); });
        }));
        if (ex == Exch::ranks) return jh_comm_allreduce_normsq(normsq);
        *normsq = 0.0;                                                   // team: the host adds the members' accumulators
        for (int k = M - 1; k >= 0; k--) {
            JH_TRY(use(k));
            JH_TRY(jh_comm_join());
            double part = 0.0;
            JH_TRY(jh_normsq_read(&part));
            *normsq += part;
        }
        return JH_OK;
    }
    // the members' streams have finished: the caller's temporaries may die
    int sync_all() const
    {
        for (int k = 0; k < M; k++) {
            jh_context *ck = jh_ctx_by_id(ops[k]->ctx);
            if (ck) { JH_TRY(use(k)); JH_CHECK_HIP(hipStreamSynchronize(ck->stream)); }
        }
        return JH_OK;
    }
};

static std::vector<Passes> passes_of(const Shards &sh, const jh_chain *ch)
{
    std::vector<Passes> pass((size_t)sh.M);
    for (int k = 0; k < sh.M; k++) { pass[k].op = sh.ops[k]; pass[k].ch = ch; pass[k].grid = !ch && !sh.tall(k); }
    return pass;
}

// x <- 0 unless it is a warm start ;  *bsq = ||b||^2 over the shards
static int start_norm_b(Shards &sh, int use_x0, double *bsq)
{
    for (int k = 0; k < sh.M; k++) {
        if (!use_x0) JH_TRY(jh_fill(sh.xs[k], 0.0, 0.0));
        double nrm = 0.0;
        JH_TRY(jh_norm(sh.rhs[k], 2.0, &nrm));                            // ||b|| (this shard's rows)
        sh.locals[k] = nrm * nrm;
    }
    return sh.sum(sh.locals, bsq);
}

// ... and the residual the iterations start from, in the right-hand side's storage: rhs <- b - A x0 on a warm start ;  *rsq = ||rhs||^2
static int start_residual(Shards &sh, std::vector<Passes> &pass, int use_x0, double *bsq, double *rsq)
{
    JH_TRY(start_norm_b(sh, use_x0, bsq));
    *rsq = *bsq;
    if (!use_x0) return JH_OK;
    for (int k = 0; k < sh.M; k++) JH_TRY(pass[k].fwd_axpby(sh.rhs[k], sh.xs[k], -1.0, 1.0, &sh.locals[k]));
    return sh.sum(sh.locals, rsq);
}

// LSQR's start-up: beta u = b - A x0, alpha v = A'u, w = v, and the scalar state before the first iteration
static int lsqr_start(Shards &sh, std::vector<Passes> &pass, std::vector<DomVecs<3>> &t, int use_x0, double damp, double atol, double btol, double conlim,
                      int maxiter, int force_maxiter, LsqrDev *h)
{
    const int M = sh.M;
    double bsq = 0.0, usq = 0.0;
    JH_TRY(start_residual(sh, pass, use_x0, &bsq, &usq));
    const double beta = std::sqrt(usq);
    double alpha = 0.0;
    if (beta > 0) {                                                      // v = A'u / beta
        for (int k = 0; k < M; k++) JH_TRY(pass[k].adjoint(t[k][ATU], sh.rhs[k]));
        JH_TRY(sh.grouped([&](int k) { return jh_comm_allreduce_sum(t[k][ATU]); }));
        for (int k = 0; k < M; k++) JH_TRY(lincomb1(t[k][V], 1.0 / beta, t[k][ATU]));
        JH_TRY(jh_norm(t[0][V], 2.0, &alpha));                           // replicas are identical: member 0 speaks for all
    } else {
        for (int k = 0; k < M; k++) JH_TRY(jh_copy(t[k][V], sh.xs[k]));
    }
    for (int k = 0; k < M; k++) {
        if (alpha > 0) JH_TRY(lincomb1(t[k][V], 1.0 / alpha, t[k][V]));
        JH_TRY(jh_copy(t[k][W], t[k][V]));
    }
    double wnorm = 0.0;                                                  // ||w_k||, needed one iteration after w_k is written
    JH_TRY(jh_norm(t[0][W], 2.0, &wnorm));
    *h = lsqr_state_init(alpha, beta, std::sqrt(bsq), wnorm, damp, atol, btol, conlim, maxiter, force_maxiter);
    return JH_OK;
}

// The host-driven loop: the recurrences are lsqr_s1 / lsqr_s2 above, applied here to a host copy of the state between the launches -- two host
// synchronisations per iteration (the step's ||u||^2, the v update's ||v||^2)
static int lsqr_impl(const int M, const jh_blockop *const *ops, jh_bvec *const *us, jh_bvec *const *xs, int use_x0, double damp, double atol,
                     double btol, double conlim, int maxiter, int force_maxiter, jh_lsqr_result *res, double *history, const Exch ex,
                     const jh_chain *ch = nullptr, const bool grid_ok = false)
{
    Shards sh("jh_lsqr_solve", M, ops, us, xs, ex);
    // a chain; rows off the 16-byte pack grid are fine (jh_blockop_tall_step_ok): the pipelined exchange cuts the DOMAIN at 16-byte bounds, and the last
    // range may end with the vector; grid_ok (jh_lsqr_solve: one GPU, unpartitioned): an N x (2 .. 4) grid of equal elementwise blocks on its one-pass
    // step (jh_grid_step.hip)
    JH_TRY(sh.init(res, maxiter, [&](int k) { return ch || sh.tall(k) || (grid_ok && jhb::grid_step_ok(ops[k], us[k]->data, xs[k]->data, xs[k]->data)); },
                   "a tall operator of >= 2 equal elementwise rows"));
    std::vector<Passes> pass = passes_of(sh, ch);
    std::vector<DomVecs<3>> t((size_t)M);
    const int dtype = sh.dtype, grid = dom_grid(sh.n, dtype);
    for (int k = 0; k < M; k++) {
        JH_TRY(sh.use(k));
        JH_TRY(t[k].create(sh.n, dtype, 2 * (size_t)grid + 2));           // 2 x grid per-workgroup partials + 2 result slots
    }
    auto parts_v = [&](int k) { return t[k].parts; };
    auto parts_w = [&](int k) { return t[k].parts + grid; };
    double *slot_v = t[0].parts + 2 * grid, *slot_w = slot_v + 1;        // member 0 folds and reports the domain-side norms
    JH_TRY(sh.use(0));
    jh_context &c = jh_ctx();                                            // member 0's context: its stream carries the read-backs
    *res = jh_lsqr_result{};
    LsqrDev h;
    JH_TRY(lsqr_start(sh, pass, t, use_x0, damp, atol, btol, conlim, maxiter, force_maxiter, &h));
    if (h.arnorm != 0) {
        while (h.itn < maxiter) {
            // ---- bidiagonalisation in one pass:  beta*u = A v - alpha*u ;  alpha*v = A'u - beta*v
            double s2 = 0.0;
            if (ex != Exch::none) JH_TRY(sh.ranged_step([&](int k) { return t[k][V]; }, [&](int k) { return t[k][ATU]; }, h.coef_step[0], h.coef_step[1], &s2));
            else JH_TRY(pass[0].step(us[0], t[0][V], t[0][ATU], h.coef_step[0], h.coef_step[1], &s2));
            // the step's read-back synchronised member 0's stream: ||w||^2 of the previous iteration (copied below) has landed in red_host[5]
            lsqr_s1(&h, s2, c.red_host + 5);
            if (!h.skipv) {
                for (int k = M - 1; k >= 0; k--) {                       // v <- A'(u_hat)/beta - beta v, ||v||^2 (member 0 last: it reports)
                    JH_TRY(sh.use(k));
                    JH_TRY(launch_vhat(dtype, t[k][V], t[k][ATU], h.coef_vhat[0], h.coef_vhat[1], parts_v(k), grid));
                }
                hipLaunchKernelGGL(k_lsqr_fold, dim3(1), dim3(256), 0, c.stream, parts_v(0), grid, slot_v);
                JH_CHECK_HIP(hipGetLastError());
                JH_CHECK_HIP(hipMemcpyAsync(c.red_host + 4, slot_v, sizeof(double), hipMemcpyDeviceToHost, c.stream));
                JH_CHECK_HIP(hipStreamSynchronize(c.stream));
            }
            lsqr_s2(&h, c.red_host[4], history);
            if (h.done) break;                                           // underflow far past convergence: x is left at its last finite update
            for (int k = M - 1; k >= 0; k--) {                           // v normalised; x += t1 w; w = v + t2 w; ||w||^2
                JH_TRY(sh.use(k));
                JH_TRY(launch_xw(dtype, t[k][V], xs[k], t[k][W], h.coef_xw[0], h.coef_xw[1], h.coef_xw[2], parts_w(k), grid));
            }
            hipLaunchKernelGGL(k_lsqr_fold, dim3(1), dim3(256), 0, c.stream, parts_w(0), grid, slot_w);
            JH_CHECK_HIP(hipGetLastError());
            JH_CHECK_HIP(hipMemcpyAsync(c.red_host + 5, slot_w, sizeof(double), hipMemcpyDeviceToHost, c.stream));   // read after the next sync
            if (h.pending) break;
        }
    }
    lsqr_result_from(h, res);
    return sh.sync_all();                                                // the temporaries die here
}

// The graph-replayed loop for ONE small operator in one context (see LsqrDev above).  *took = false: not eligible, nothing was
// touched, the caller runs lsqr_impl.
static int lsqr_graph_impl(const jh_blockop *op, jh_bvec *u, jh_bvec *x, int use_x0, double damp, double atol, double btol, double conlim,
                           int maxiter, int force_maxiter, jh_lsqr_result *res, double *history, bool *took)
{
    *took = false;
    JH_TRY(jh_enter(op, u, x));
    jh_context &c = jh_ctx();
    c.last_lsqr_graph = 0;
    if (!c.lsqr_graph || !op || !u || !x || !res || maxiter < 1) return JH_OK;
    if (!jh_blockop_tall_step_ok(op, u->data, x->data)) return JH_OK;       // (rows off the 16-byte pack grid too: the plain step's MIXED instantiations)
    // one plain launch per step: no split walk (pick_adj_parts), no row-chunked launches; and only where launches and host
    // round trips matter: a pass over the operator and u below 1 GiB
    if (!(jh_bidiag_step_parts(op) == 1 && c.adj_rows_per_launch == 0)) return JH_OK;
    const int dtype = x->dtype;
    const int64_t n = x->length;
    // (late round 4: up to 2 GiB per pass when the blocks are below 16 MiB -- the sizes whose step has one way to walk, so nothing is lost by not measuring
    // it per operator: 64 x 128^3 317 -> 305 us per iteration; knob lsqr_graph = 2: any size)
    const double pass_bytes = 3.0 * (double)op->nrow * (double)n * (double)jh_dtype_size(dtype);
    if (c.lsqr_graph < 2 && !(pass_bytes < (double)(1ull << 30) || (pass_bytes < (double)(2ull << 30) && (double)n * (double)jh_dtype_size(dtype) < (double)(16u << 20))))
        return JH_OK;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(c.stream, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) return JH_OK;
    *took = true;

    Shards sh("jh_lsqr_solve", 1, &op, &u, &x, Exch::none);
    JH_TRY(sh.init(res, maxiter, [](int) { return true; }, ""));
    std::vector<Passes> pass = passes_of(sh, nullptr);
    std::vector<DomVecs<3>> tv(1);
    const int grid = dom_grid(n, dtype);
    JH_TRY(tv[0].create(n, dtype, 2 * (size_t)grid + 2));
    const DomVecs<3> &t = tv[0];
    double *parts_v = t.parts, *parts_w = t.parts + grid, *slot_v = t.parts + 2 * grid, *slot_w = slot_v + 1;
    *res = jh_lsqr_result{};
    LsqrDev h;
    JH_TRY(lsqr_start(sh, pass, tv, use_x0, damp, atol, btol, conlim, maxiter, force_maxiter, &h));   // one shard, no exchange
    lsqr_result_from(h, res);
    if (h.arnorm == 0) return JH_OK;                                      // (istop = itn = 0, like lsqr_impl)

    // ---- device state
    struct Dev {
        LsqrDev *st = nullptr;
        double *hist = nullptr;
        hipGraph_t graph = nullptr;
        hipGraphExec_t exec = nullptr;
        ~Dev()
        {
            if (exec) (void)hipGraphExecDestroy(exec);
            if (graph) (void)hipGraphDestroy(graph);
            if (st) (void)hipFree(st);
            if (hist) (void)hipFree(hist);
        }
    } d;
    JH_CHECK_HIP(jh_device_malloc(c.device, (void **)&d.st, sizeof(LsqrDev)));
    JH_CHECK_HIP(jh_device_malloc(c.device, (void **)&d.hist, sizeof(double) * 2 * (size_t)maxiter));
    JH_CHECK_HIP(hipMemcpyAsync(d.st, &h, sizeof(h), hipMemcpyHostToDevice, c.stream));
    JH_CHECK_HIP(hipStreamSynchronize(c.stream));                        // `h` is a stack object

    // one iteration, enqueued on the context's stream: eagerly the first time (workspaces get their size), captured the second
    auto iteration = [&]() -> int {
        JH_TRY(jh_normsq_reset());
        c.step_coef_dev = d.st->coef_step;
        c.step_done_dev = &d.st->done;
        const int st_ = jh_blockop_bidiag_step_range(op, u, t[V], t[ATU], 1.0, 0.0, 0, n, nullptr);     // (alpha, beta) come from the device
        c.step_coef_dev = nullptr;
        c.step_done_dev = nullptr;
        JH_TRY(st_);
        hipLaunchKernelGGL(k_lsqr_s1, dim3(1), dim3(1), 0, c.stream, d.st, (const double *)(c.red_dev + JH_NORMSQ_SLOT), (const double *)slot_w);
        JH_TRY(launch_vhat_dev(dtype, t[V], t[ATU], d.st, parts_v, grid));
        hipLaunchKernelGGL(k_lsqr_fold, dim3(1), dim3(256), 0, c.stream, (const double *)parts_v, grid, slot_v);
        hipLaunchKernelGGL(k_lsqr_s2, dim3(1), dim3(1), 0, c.stream, d.st, (const double *)slot_v, d.hist);
        JH_TRY(launch_xw_dev(dtype, t[V], x, t[W], d.st, parts_w, grid));
        hipLaunchKernelGGL(k_lsqr_fold, dim3(1), dim3(256), 0, c.stream, (const double *)parts_w, grid, slot_w);
        hipLaunchKernelGGL(k_lsqr_s3, dim3(1), dim3(1), 0, c.stream, d.st);
        JH_CHECK_HIP(hipGetLastError());
        return JH_OK;
    };
    // the same iteration with the scalar steps fused into the folds (five nodes): possible when the step's partial sums fit ONE
    // fold launch (k_sum_partials' single-level form, <= 8192 workgroups) -- known after the eager iteration
    auto iteration_fused = [&]() -> int {
        c.step_coef_dev = d.st->coef_step;
        c.step_done_dev = &d.st->halt;
        c.step_skip_fold = 1;
        const int st_ = jh_blockop_bidiag_step_range(op, u, t[V], t[ATU], 1.0, 0.0, 0, n, nullptr);
        c.step_coef_dev = nullptr;
        c.step_done_dev = nullptr;
        c.step_skip_fold = 0;
        JH_TRY(st_);
        hipLaunchKernelGGL(k_lsqr_fold_s1, dim3(1), dim3(256), 0, c.stream, (const double *)c.part_dev, c.last_step_parts, d.st, (const double *)parts_w, grid, slot_w);
        JH_TRY(launch_vhat_dev(dtype, t[V], t[ATU], d.st, parts_v, grid));
        hipLaunchKernelGGL(k_lsqr_fold_s2, dim3(1), dim3(256), 0, c.stream, (const double *)parts_v, grid, d.st, d.hist);
        JH_TRY(launch_xw_dev(dtype, t[V], x, t[W], d.st, parts_w, grid));
        JH_CHECK_HIP(hipGetLastError());
        return JH_OK;
    };
    struct Flags { int itn, istop, done, pending; } fl{};
    auto read_flags = [&]() -> int {
        JH_CHECK_HIP(hipMemcpyAsync(&fl, &d.st->itn, sizeof(fl), hipMemcpyDeviceToHost, c.stream));
        JH_CHECK_HIP(hipStreamSynchronize(c.stream));
        return JH_OK;
    };
    JH_TRY(iteration());                                                  // iteration 1, eager
    JH_TRY(read_flags());
    int64_t replays = 0;
    if (!fl.done) {
        const bool fused = c.last_step_parts > 0 && c.last_step_parts <= 8192;
        // round 4: EIGHT iterations per graph (finished solves replay as no-ops): one hipGraphLaunch costs the host 10-16 us
        const int per_graph = maxiter < 8 ? maxiter : 8;
        JH_CHECK_HIP(hipStreamBeginCapture(c.stream, hipStreamCaptureModeRelaxed));   // other host threads (other contexts) keep working meanwhile
        int st_ = JH_OK;
        for (int k = 0; k < per_graph && st_ == JH_OK; k++) st_ = fused ? iteration_fused() : iteration();
        hipError_t e = hipStreamEndCapture(c.stream, &d.graph);
        if (st_ != JH_OK) return st_;
        JH_CHECK_HIP(e);
        JH_CHECK_HIP(hipGraphInstantiate(&d.exec, d.graph, nullptr, nullptr, 0));
        while (!(fl.done || (fused && fl.pending))) {                     // two graphs between two looks at the flags (five nodes: `pending` ends the solve)
            for (int k = 0; k < 2; k++) JH_CHECK_HIP(hipGraphLaunch(d.exec, c.stream));
            replays += 2;
            JH_TRY(read_flags());
        }
    }
    c.last_lsqr_graph = replays;
    JH_CHECK_HIP(hipMemcpyAsync(&h, d.st, sizeof(h), hipMemcpyDeviceToHost, c.stream));
    JH_CHECK_HIP(hipStreamSynchronize(c.stream));
    if (history && h.itn > 0) {                                           // (on the context's stream: a legacy-stream copy would disturb another thread's capture)
        JH_CHECK_HIP(hipMemcpyAsync(history, d.hist, sizeof(double) * 2 * (size_t)h.itn, hipMemcpyDeviceToHost, c.stream));
        JH_CHECK_HIP(hipStreamSynchronize(c.stream));
    }
    lsqr_result_from(h, res);
    return JH_OK;
}

// ---- what the entry points of the three solvers check alike; `who` is the solver's plain entry, whose name the messages extend ----
// jh_*_solve_partitioned: the communicator is the one of the handles' context.  One rank: nothing to exchange (jh_comm_init_rank is then optional, so a
// one-GPU run of partitioned host code works); the knob force_dist runs the exchange all the same (validation of the pipelined path with a one-rank
// communicator)
static int partitioned_exchange(const char *who, const jh_blockop *op, const jh_bvec *u, const jh_bvec *x, Exch *ex)
{
    JH_TRY(jh_enter(op, u, x));
    int nranks = 1, rank = 0, has_comm = 0;
    (void)jh_comm_info(&nranks, &rank);
    (void)jh_comm_exists(&has_comm);
    if (has_comm == 2 && (nranks > 1 || jh_ctx().force_dist))
        return jh_fail(JH_ERR_UNSUPPORTED, "%s_partitioned: this context is a member of a single-process team (jh_comm_init_all): "
                       "%s_team takes all the members' shards in one call", who, who);
    *ex = (nranks > 1 || (has_comm && jh_ctx().force_dist)) ? Exch::ranks : Exch::none;
    return JH_OK;
}

// jh_*_solve_team: member k's handles live in member k's context of a team of n
static int team_members_ok(const char *who, int n, const jh_blockop *const *ops, jh_bvec *const *us, jh_bvec *const *xs)
{
    JH_REQUIRE(n >= 1 && n <= JH_MAX_CTX && ops && us && xs, "%s_team: need 1..%d members", who, JH_MAX_CTX);
    for (int k = 0; k < n; k++) {
        JH_REQUIRE(ops[k] && us[k] && xs[k], "%s_team: null handle of member %d", who, k);
        JH_TRY(jh_enter(ops[k], us[k], xs[k]));
        int nranks = 1, rank = 0, has_comm = 0;
        (void)jh_comm_info(&nranks, &rank);
        (void)jh_comm_exists(&has_comm);
        JH_REQUIRE(has_comm == 2 && nranks == n && rank == k, "%s_team: the handles of member %d must live in member %d's context of a team of %d "
                   "(jh_comm_init_all); found %s, rank %d of %d", who, k, k, n, has_comm == 2 ? "a team" : "no team", rank, nranks);
    }
    return JH_OK;
}

extern "C" int jh_lsqr_solve(const jh_blockop *op, jh_bvec *u, jh_bvec *x, int use_x0, double damp, double atol, double btol, double conlim,
                             int maxiter, int force_maxiter, jh_lsqr_result *res, double *history)
{
    bool took = false;
    JH_TRY(lsqr_graph_impl(op, u, x, use_x0, damp, atol, btol, conlim, maxiter, force_maxiter, res, history, &took));   // small operators
    if (took) return JH_OK;
    return lsqr_impl(1, &op, &u, &x, use_x0, damp, atol, btol, conlim, maxiter, force_maxiter, res, history, Exch::none, nullptr, true);
}

extern "C" int jh_lsqr_solve_partitioned(const jh_blockop *op, jh_bvec *u, jh_bvec *x, int use_x0, double damp, double atol, double btol,
                                         double conlim, int maxiter, int force_maxiter, jh_lsqr_result *res, double *history)
{
    Exch ex = Exch::none;
    JH_TRY(partitioned_exchange("jh_lsqr_solve", op, u, x, &ex));
    return lsqr_impl(1, &op, &u, &x, use_x0, damp, atol, btol, conlim, maxiter, force_maxiter, res, history, ex);
}

// ONE process, a team of n member contexts (jh_comm_init_all): member k holds ops[k] (its block rows), us[k] (its rows of the
// right-hand side; overwritten) and xs[k] (its replica of the solution).  The same loop as jh_lsqr_solve_partitioned, the
// members' kernels enqueued one after the other, their ranged all-reduces grouped, scalars added on the host.
extern "C" int jh_lsqr_solve_team(int n, const jh_blockop *const *ops, jh_bvec *const *us, jh_bvec *const *xs, int use_x0, double damp, double atol,
                                  double btol, double conlim, int maxiter, int force_maxiter, jh_lsqr_result *res, double *history)
{
    JH_TRY(team_members_ok("jh_lsqr_solve", n, ops, us, xs));
    return lsqr_impl(n, ops, us, xs, use_x0, damp, atol, btol, conlim, maxiter, force_maxiter, res, history, Exch::team);
}

// ------------------------------------------------------------------ CGLS (round 3; SURVEY section 8 f-1 "LSQR/CGLS") ------------------------
// Conjugate gradients on the normal equations (Hestenes & Stiefel 1952; Bjorck, "Numerical Methods for Least Squares Problems",
// 1996, algorithm 7.4.1 "CGLS"), min ||A x - b||^2 + damp^2 ||x||^2, over the same shards and exchange modes as lsqr_impl.  The
// reference ships no solver (src/Jets.jl:1143-1152 points at IterativeSolvers.jl, un-vendored), so this is the published recurrence,
// checked against the fp64 CPU CGLS of oracle/cgls_ref.py.
//
//   r = b - A x0 ;  s = A'r - damp^2 x ;  p = s ;  gamma = ||s||^2
//   repeat:  delta = ||A p||^2 + damp^2 ||p||^2 ;  alpha = gamma / delta ;  x += alpha p ;  r -= alpha A p
//            s = A'r - damp^2 x ;  gamma' = ||s||^2 ;  p = s + (gamma'/gamma) p
//
// The textbook loop keeps q = A p in a range-sized vector (64 GiB at the headline size) and moves 7 N n s bytes per iteration
// through the two fused halves (q = A p with ||q||^2: 2 N n s; r -= alpha q: 3 N n s; s = A'r: 2 N n s).  Here an iteration is TWO
// passes and no q:   ||A p||^2 = <p, A'A p>  from the fused normal operator (jh_blockop_normal_mul: reads the coefficients only,
// N n s bytes; the inner product is a domain-sized fp64 reduction), then ONE pass of the Golub-Kahan step kernel
// (jh_blockop_bidiag_step with (alpha, beta) = (-alpha_k, 1)):  r <- r - alpha_k A p,  ||r||^2  and  A'r  together, 3 N n s bytes.
// 4 N n s bytes per iteration against LSQR's 3 N n s.  Partitioned: the first pass needs a SCALAR exchange only (every shard's
// <p, A_k'A_k p>), the second is LSQR's pipelined step (ranged all-reduces of A'r under the kernels, one host synchronisation).
static int cgls_impl(const int M, const jh_blockop *const *ops, jh_bvec *const *us, jh_bvec *const *xs, int use_x0, double damp, double atol,
                     double btol, int maxiter, int force_maxiter, jh_lsqr_result *res, double *history, const Exch ex,
                     const jh_chain *ch = nullptr, const bool grid_ok = false)
{
    Shards sh("jh_cgls_solve", M, ops, us, xs, ex);
    // a chain; a tall operator (rows off the 16-byte pack grid too, as in lsqr_impl) of two rows or more; grid_ok (jh_cgls_solve: one GPU, unpartitioned): an
    // N x (2 .. 4) grid of equal elementwise blocks -- its one-pass step (jh_grid_step.hip) and its fused A'A (jh_grid_normal.hip) are both asked
    JH_TRY(sh.init(res, maxiter, [&](int k) {
        if (ch) return true;
        if (sh.tall(k)) return ops[k]->nrow >= 2;
        return grid_ok && jhb::grid_step_ok(ops[k], us[k]->data, xs[k]->data, xs[k]->data) && jhb::grid_normal_ok(ops[k], xs[k]->data, xs[k]->data);
    }, "a tall (>= 2 rows) operator of equal elementwise rows"));
    std::vector<Passes> pass = passes_of(sh, ch);
    std::vector<DomVecs<3>> t((size_t)M);
    for (int k = 0; k < M; k++) {
        JH_TRY(sh.use(k));
        JH_TRY(t[k].create(sh.n, sh.dtype));
    }
    *res = jh_lsqr_result{};
    // s = A'r (already summed over the shards, in t[k][S]) - damp^2 x ;  returns ||s||^2 (member 0 speaks for all: replicas are identical)
    auto finish_s = [&](double *gamma) -> int {
        for (int k = 0; k < M; k++)
            if (damp != 0.0) JH_TRY(lincomb2(t[k][S], 1.0, t[k][S], -damp * damp, xs[k]));
        double nrm = 0.0;
        JH_TRY(jh_norm(t[0][S], 2.0, &nrm));
        *gamma = nrm * nrm;
        return JH_OK;
    };
    std::vector<double> &locals = sh.locals;
    jh_context *const trace_ctx = jh_ctx_by_id(ops[0]->ctx);              // knob cgls_trace / read-only last_cgls_overlaps live in member 0's context
    if (trace_ctx) trace_ctx->last_cgls_overlaps = -1;

    double s2 = 0.0, rr = 0.0;                                            // ||b||^2 ;  ||r||^2, r <- b - A x0 in the right-hand side's storage
    JH_TRY(start_residual(sh, pass, use_x0, &s2, &rr));
    const double bnorm = std::sqrt(s2);
    for (int k = 0; k < M; k++) JH_TRY(pass[k].adjoint(t[k][S], us[k]));                     // s = A'r
    JH_TRY(sh.grouped([&](int k) { return jh_comm_allreduce_sum(t[k][S]); }));
    double gamma = 0.0;
    JH_TRY(finish_s(&gamma));
    for (int k = 0; k < M; k++) JH_TRY(jh_copy(t[k][P], t[k][S]));
    const double gamma0 = gamma;
    double xnorm = 0.0;
    int itn = 0, istop = 0;
    if (gamma > 0) {
        while (itn < maxiter) {
            itn++;
            // ---- pass 1: delta = <p, A'A p> + damp^2 ||p||^2 (every shard's share of the quadratic form, then a scalar sum)
            // every member's pass and its inner product are ENQUEUED before the first wait: the members' GPUs run side by side (round 3
            // waited for member k's dot before member k + 1's kernel was even launched: M passes one after the other)
            const bool trace = itn == 1 && M > 1 && trace_ctx && trace_ctx->cgls_trace;   // tests: event timestamps of the first iteration's pass 1
            std::vector<hipEvent_t> tev(trace ? (size_t)(2 * M) : 0, nullptr);
            auto stamp = [&](int k, int which) -> int {
                if (!trace) return JH_OK;
                JH_TRY(sh.use(k));
                JH_CHECK_HIP(hipEventCreate(&tev[(size_t)(2 * k + which)]));
                JH_CHECK_HIP(hipEventRecord(tev[(size_t)(2 * k + which)], jh_ctx().stream));
                return JH_OK;
            };
            for (int k = 0; k < M; k++) {
                JH_TRY(stamp(k, 0));
                JH_TRY(pass[k].normal(t[k][Y], t[k][P]));
                JH_TRY(jh_dot_begin(t[k][P], t[k][Y]));
                JH_TRY(stamp(k, 1));
            }
            for (int k = 0; k < M; k++) {
                double re = 0.0, im = 0.0;
                JH_TRY(jh_dot_end(t[k][P], &re, &im));
                locals[k] = re;
            }
            if (trace) {                                                  // member k + 1 began before member k had finished?  (members of ONE device: one clock)
                int64_t overlaps = 0;
                for (int k = 0; k + 1 < M; k++) {
                    float ms = 0.f;                                       // from k's end to (k + 1)'s begin: negative when they overlap
                    if (hipEventElapsedTime(&ms, tev[(size_t)(2 * k + 1)], tev[(size_t)(2 * k + 2)]) == hipSuccess && ms < 0.f) overlaps++;
                }
                (void)hipGetLastError();
                trace_ctx->last_cgls_overlaps = overlaps;
                for (hipEvent_t e : tev)
                    if (e) (void)hipEventDestroy(e);
            }
            double delta = 0.0;
            JH_TRY(sh.sum(locals, &delta));
            if (damp != 0.0) {
                double pn = 0.0;
                JH_TRY(jh_norm(t[0][P], 2.0, &pn));
                delta += damp * damp * pn * pn;
            }
            if (!(delta > 0) || !std::isfinite(delta)) {                  // breakdown: p in the null space (or the recurrences have underflowed)
                istop = 6;
                itn--;
                break;
            }
            const double alpha = gamma / delta;
            for (int k = 0; k < M; k++) JH_TRY(lincomb2(xs[k], 1.0, xs[k], alpha, t[k][P]));   // x += alpha p
            // ---- pass 2: r <- r - alpha A p, ||r||^2 and A'r in ONE pass over the operator and r
            if (ex != Exch::none) JH_TRY(sh.ranged_step([&](int k) { return t[k][P]; }, [&](int k) { return t[k][S]; }, -alpha, 1.0, &rr));
            else JH_TRY(pass[0].step(us[0], t[0][P], t[0][S], -alpha, 1.0, &rr));
            double gamma_new = 0.0;
            JH_TRY(finish_s(&gamma_new));
            const double bk = gamma_new / gamma;
            for (int k = 0; k < M; k++) JH_TRY(lincomb2(t[k][P], 1.0, t[k][S], bk, t[k][P]));   // p = s + beta p
            gamma = gamma_new;
            const double rnorm = std::sqrt(rr), arnorm = std::sqrt(gamma);
            if (history) { history[2 * (itn - 1)] = rnorm; history[2 * (itn - 1) + 1] = arnorm; }
            if (itn >= maxiter) istop = 7;
            if (arnorm <= atol * std::sqrt(gamma0)) istop = 2;            // ||A'r - damp^2 x|| small against its starting value
            if (rnorm <= btol * bnorm) istop = 1;                         // ||r|| small against ||b||
            if (istop && !(force_maxiter && itn < maxiter && gamma > 0)) break;
        }
    }
    JH_TRY(jh_norm(xs[0], 2.0, &xnorm));
    res->istop = istop;
    res->itn = itn;
    res->r1norm = std::sqrt(rr);
    res->r2norm = std::sqrt(rr + damp * damp * xnorm * xnorm);
    res->anorm = 0.0;                                                     // (LSQR's running estimates have no counterpart here)
    res->acond = 0.0;
    res->arnorm = std::sqrt(gamma);
    res->xnorm = xnorm;
    return sh.sync_all();                                                 // the temporaries die here
}

// ------------------------------------------------------------------ CGLS and CG on the normal equations for SMALL operators (round 4) -----
// The loops above (cgls_impl, cgnr_impl below) return to the host two or three times per iteration for a scalar and launch about a dozen
// small kernels: for an operator whose fused A'A takes 11 us that is 60 us per iteration (64 x 64^3, profiles/bench_cgnr_sizes_r03.txt).
// Here -- as lsqr_graph_impl does for LSQR -- the scalars of the recurrences are a struct in device memory (jh_cg_dev), the one-thread
// epilogues of two fold kernels update it, every vector kernel reads its coefficients from it and becomes a no-op once the solve has
// finished, so one iteration has fixed launch parameters, is captured ONCE as a hipGraph and replayed:
//   CG on the normal equations, 3 nodes:  k_cg_normal  [p <- s + bk p ; y = (A'A + damp^2) p ; partial <p, y>]      (jh_tall.hip)
//                                         k_cg_xs      [fold of <p, y> -> alpha, breakdown ; x += alpha p ; s -= alpha y ; partial ||s||^2]
//                                         k_cg_fold    [gamma', beta, ||r|| by recurrence, history, stopping rules]
//   CGLS, 5 nodes:  k_cg_normal ; k_cg_fold ; the one-pass step r <- r - alpha A p, A'r, partial ||r||^2 (coefficients from the device) ;
//                   k_cgls_xs [x += alpha p ; s -= damp^2 x ; partial ||s||^2] ; k_cg_fold
// The two scalar updates (cg_s1, cg_s2) are `__host__ __device__` functions: with the knob lsqr_graph = 0 the SAME kernels run eagerly
// and the host applies the same two functions between them (one read-back each) -- the host-driven form of this loop, whose iterates the
// replayed graph reproduces bit for bit (tests/test_gpu_graphs.py).  Operators of 1 GiB and more per pass, partitioned and team solves
// keep cgls_impl / cgnr_impl (their tuned kernels, split walks and pipelined exchange); both forms are checked against the fp64 CPU CGLS.
// which == 1: the sum of `partials` is <p, (A'A + damp^2) p>; which == 2: the sum of `partials` is ||s||^2 and (CGLS) the sum of
// `rparts` the step's ||r||^2 (k_sum_partials' single-level order: `0.0 + r`).  on_device: apply the scalar update here, else leave
// the sums in out[0], out[1] for the host.
__global__ __launch_bounds__(256) void k_cg_fold(const double *__restrict__ partials, int64_t nparts, const double *__restrict__ rparts, int64_t nrparts,
                                                 jh_cg_dev *st, double *__restrict__ history, double *__restrict__ out, int which, int on_device)
{
    // every load is issued before anything depends on one (the state, the flag and the partials travel together: a dependent launch of
    // a few hundred bytes is all latency); a finished solve changes nothing at the end instead of returning at the start
    jh_cg_dev loc;
    if (threadIdx.x == 0) loc = *st;
    const int done = st->done;
    const double v = jh_strided_sum256(partials, nparts), w = rparts ? jh_strided_sum256(rparts, nrparts) : 0.0;
    const double r = wg_sum_value<256>(v);
    double r2 = 0.0;
    if (rparts) {
        __syncthreads();                                                  // (wg_sum_value's staging array is reused)
        r2 = 0.0 + wg_sum_value<256>(w);
    }
    if (threadIdx.x == 0 && !done) {
        if (!on_device) { out[0] = r; out[1] = r2; }
        else {
            if (which == 1) cg_s1(&loc, r);
            else cg_s2(&loc, r, r2, history);
            *st = loc;
        }
    }
}

// fold_n != nullptr (CG on the normal equations, graph form): the fold of the <p, y> partials and the first scalar update are done HERE
// instead of in a launch of their own -- every workgroup adds the same partials in the same order (the same bits everywhere) and forms
// alpha = gamma / <p, y> itself (cg_s1 writes neither gamma nor damp2; what it does write -- itn, delta, alpha, the step coefficients and,
// on a breakdown, istop and done -- no other workgroup's result depends on: on a breakdown every workgroup returns without an update,
// whether it saw `done` or found the breakdown itself); workgroup 0 records the update.  Three graph nodes per iteration instead of
// four: a dependent launch costs 4-5 us even when it does nothing.
template <typename S>
__global__ __launch_bounds__(256) void k_cg_xs(S *__restrict__ x, S *__restrict__ s, const S *__restrict__ p, const S *__restrict__ y, int64_t n,
                                               jh_cg_dev *st, double *__restrict__ partials, const double *__restrict__ fold_n, int64_t nfold)
{
    // the first element's operands, the state and the partials to fold are all loaded before anything is decided (see k_cg_fold)
    const int64_t i0 = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
    const int64_t j0 = i0 < n ? i0 : 0;
    S x0 = x[j0], s0 = s[j0], p0 = p[j0], y0 = y ? y[j0] : (S)0;
    const int done = st->done;
    double alpha_d = st->alpha;
    const double gamma = st->gamma, damp2 = st->damp2;
    const double v = fold_n ? jh_strided_sum256(fold_n, nfold) : 0.0;
    asm volatile("" : "+v"(x0), "+v"(s0), "+v"(p0), "+v"(y0));             // (keeps the loads above the branches below)
    if (fold_n) {
        const double pap = wg_sum_value<256>(v);
        if (done) return;
        if (blockIdx.x == 0 && threadIdx.x == 0) cg_s1(st, pap);          // itn, delta, alpha (= gamma / pap), or the breakdown (see above)
        if (!(pap > 0) || !((pap - pap) == 0.0)) return;                  // breakdown: nothing is updated (every workgroup decides alike)
        alpha_d = gamma / pap;
    } else if (done) {
        return;
    }
    const S alpha = (S)alpha_d, nalpha = (S)(-alpha_d), nd2 = (S)(-damp2);
    const bool damped = damp2 != 0.0;
    double nrm = 0.0;
    for (int64_t i = i0; i < n; i += stride) {
        if (i != i0) { x0 = x[i]; s0 = s[i]; p0 = p[i]; y0 = y ? y[i] : (S)0; }
        const S ap = alpha * p0;
        const S xn = x0 + ap;
        x[i] = xn;
        S sn = s0;
        if (y) {
            const S ay = nalpha * y0;
            sn = sn + ay;
            s[i] = sn;
        } else if (damped) {
            const S dx = nd2 * xn;
            sn = sn + dx;
            s[i] = sn;
        }
        nrm += (double)sn * (double)sn;
    }
    wg_sum_to<256>(nrm, partials + blockIdx.x);
}

static inline int64_t n_packs_of(const jh_blockop *op) { return op->col_len[0] * (int64_t)jh_dtype_size(op->dtype) / 16; }

static int cg_dev_impl(const jh_blockop *op, jh_bvec *b, jh_bvec *x, int use_x0, double damp, double atol, double btol, int maxiter, int force_maxiter,
                       jh_lsqr_result *res, double *history, const bool cgls, bool *took)
{
    *took = false;
    JH_REQUIRE(op && b && x && res, "jh_cg*_solve: null argument");
    JH_REQUIRE(maxiter >= 0, "jh_cg*_solve: maxiter must be >= 0");
    JH_TRY(jh_enter(op, b, x));
    jh_context &c = jh_ctx();
    if (c.cg_dev == 0 || maxiter < 1) return JH_OK;
    if (!(op->tall && op->all_diag) || !jh_blockop_tall_step_ok(op, b->data, x->data) || op->nrow < 2) return JH_OK;   // (rows off the 16-byte pack grid too)
    // one plain launch per pass: CGLS' second pass is the one-pass step; the fused A'A of this loop (k_cg_normal) walks all rows in every
    // workgroup, which fills the chip when the domain gives a workgroup per CU (many rows of tiny blocks keep the split walk of the host loop)
    const int64_t normal_wgs = (n_packs_of(op) + 255) / 256;
    if (c.adj_rows_per_launch != 0 || (cgls ? jh_bidiag_step_parts(op) != 1 : (c.adj_split > 0 || (op->nrow >= 256 && c.adj_split != 0 && normal_wgs < c.cu_count)))) return JH_OK;
    const int dtype = x->dtype;
    const int64_t n = x->length;
    // only where launches and host round trips matter (knob cg_dev = 2: any size): CGLS below 1 GiB per pass over the operator and r (2 GiB when the
    // blocks are below 16 MiB: the step then has one way to walk); CG through
    // the fused A'A up to 2 GiB of coefficients (64 x 128^3: 140 -> 111 us per iteration, 256 x 128^3: 368 -> 346; no difference from 4 GiB on)
    const double coeff_bytes = (double)op->nrow * (double)n * (double)jh_dtype_size(dtype);
    const bool cgls_small = 3.0 * coeff_bytes < (double)(1ull << 30) || (3.0 * coeff_bytes < (double)(2ull << 30) && coeff_bytes / (double)op->nrow < (double)(16u << 20));
    if (c.cg_dev < 2 && (cgls ? !cgls_small : coeff_bytes > (double)(2ull << 30))) return JH_OK;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(c.stream, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) return JH_OK;
    *took = true;
    c.last_cg_graph = 0;

    struct Work {
        jh_bvec *p = nullptr, *s = nullptr, *y = nullptr;
        double *parts = nullptr, *hist = nullptr;
        jh_cg_dev *st = nullptr;
        hipGraph_t graph = nullptr;
        hipGraphExec_t exec = nullptr;
        ~Work()
        {
            if (exec) (void)hipGraphExecDestroy(exec);
            if (graph) (void)hipGraphDestroy(graph);
            if (parts) (void)hipFree(parts);
            if (hist) (void)hipFree(hist);
            if (st) (void)hipFree(st);
            if (p) (void)jh_bvec_destroy(p);
            if (s) (void)jh_bvec_destroy(s);
            if (y) (void)jh_bvec_destroy(y);
        }
    } t;
    const int64_t len1[1] = {n};
    JH_TRY(jh_bvec_create(1, len1, dtype, &t.p));
    JH_TRY(jh_bvec_create(1, len1, dtype, &t.s));
    JH_TRY(jh_bvec_create(1, len1, dtype, &t.y));
    const bool f64 = (dtype == JH_F64 || dtype == JH_C64);
    const int64_t ns_dom = n * (jh_dtype_complex(dtype) ? 2 : 1);
    const int grid = dom_grid(n, dtype);
    const int64_t packs = (n * (int64_t)jh_dtype_size(dtype)) / 16, grid_n = (packs + 255) / 256;
    JH_CHECK_HIP(jh_device_malloc(c.device, (void **)&t.parts, sizeof(double) * ((size_t)grid_n + (size_t)grid + 2)));
    JH_CHECK_HIP(jh_device_malloc(c.device, (void **)&t.hist, sizeof(double) * 2 * (size_t)maxiter));
    JH_CHECK_HIP(jh_device_malloc(c.device, (void **)&t.st, sizeof(jh_cg_dev)));
    double *parts_n = t.parts, *parts_s = t.parts + grid_n, *slots = parts_s + grid;
    *res = jh_lsqr_result{};

    // ---- the start-up of cgls_impl / cgnr_impl (one shard, no exchange)
    if (!use_x0) JH_TRY(jh_fill(x, 0.0, 0.0));
    double nrm = 0.0;
    JH_TRY(jh_norm(b, 2.0, &nrm));
    const double s2 = nrm * nrm, bnorm = std::sqrt(s2);
    double rr = s2;
    if (cgls) {
        if (use_x0) JH_TRY(jh_blockop_mul_axpby(op, b, x, -1.0, 1.0, &rr));                 // r <- b - A x0 (in b's storage)
        JH_TRY(jh_blockop_mul_adj(op, t.s, b));                                            // s = A'r
        if (damp != 0.0) JH_TRY(lincomb2(t.s, 1.0, t.s, -damp * damp, x));
    } else {
        JH_TRY(jh_blockop_mul_adj(op, t.s, b));                                            // s = A'b
        if (use_x0) {                                                     // s = A'b - (A'A + damp^2) x0 ; ||r0||^2 = ||b||^2 - 2 Re<x0, A'b> + <x0, A'A x0>
            JH_TRY(jh_blockop_normal_mul(op, t.y, x));
            double xb = 0.0, xax = 0.0, im = 0.0;
            JH_TRY(jh_dot(x, t.s, &xb, &im));
            JH_TRY(jh_dot(x, t.y, &xax, &im));
            rr = s2 - 2.0 * xb + xax;
            if (damp != 0.0) {
                double x0n = 0.0;
                JH_TRY(jh_norm(x, 2.0, &x0n));
                rr += damp * damp * x0n * x0n;
            }
            JH_TRY(lincomb2(t.s, 1.0, t.s, -1.0, t.y));
            if (damp != 0.0) JH_TRY(lincomb2(t.s, 1.0, t.s, -damp * damp, x));
        }
    }
    JH_TRY(jh_norm(t.s, 2.0, &nrm));
    const double gamma0 = nrm * nrm;
    JH_TRY(jh_copy(t.p, t.s));
    jh_cg_dev h{};
    h.gamma = h.gamma0 = gamma0;
    h.rr = rr;
    h.bnorm = bnorm;
    h.damp2 = damp * damp;
    h.atol = atol;
    h.btol = btol;
    h.skip_p = 1;                                                         // p = s already
    h.maxiter = maxiter;
    h.force = force_maxiter ? 1 : 0;
    h.cgls = cgls ? 1 : 0;
    auto finish = [&]() -> int {
        double xnorm = 0.0;
        JH_TRY(jh_norm(x, 2.0, &xnorm));
        res->istop = h.istop;
        res->itn = h.itn;
        if (cgls) {
            res->r1norm = std::sqrt(h.rr);
            res->r2norm = std::sqrt(h.rr + damp * damp * xnorm * xnorm);
        } else {
            res->r2norm = std::sqrt(h.rr);
            const double r1sq = h.rr - damp * damp * xnorm * xnorm;
            res->r1norm = std::sqrt(r1sq > 0 ? r1sq : 0.0);
        }
        res->anorm = 0.0;
        res->acond = 0.0;
        res->arnorm = std::sqrt(h.gamma);
        res->xnorm = xnorm;
        return JH_OK;
    };
    if (!(gamma0 > 0)) return finish();
    auto push_state = [&]() -> int {
        JH_CHECK_HIP(hipMemcpyAsync(t.st, &h, sizeof(h), hipMemcpyHostToDevice, c.stream));
        JH_CHECK_HIP(hipStreamSynchronize(c.stream));                    // `h` is a stack object
        return JH_OK;
    };
    JH_TRY(push_state());

    int64_t nparts_n = 0, nparts_r = 0;
    // the first half of an iteration: the normal-equations pass and its fold;  the second: (CGLS: the step,) the vector updates, their fold
    bool fuse = false;                                                    // graph form of CG on the normal equations: the first fold inside k_cg_xs
    auto half1 = [&](int on_device) -> int {
        JH_TRY(jh_launch_cg_normal(op, t.p, t.s, t.y, t.st, parts_n, &nparts_n));
        if (fuse) return JH_OK;
        hipLaunchKernelGGL(k_cg_fold, dim3(1), dim3(256), 0, c.stream, (const double *)parts_n, nparts_n, (const double *)nullptr, (int64_t)0, t.st, t.hist, slots, 1,
                           on_device);
        JH_CHECK_HIP(hipGetLastError());
        return JH_OK;
    };
    auto half2 = [&](int on_device) -> int {
        const double *rparts = nullptr;
        if (cgls) {
            c.step_coef_dev = t.st->coef_step;
            c.step_done_dev = &t.st->done;
            c.step_skip_fold = 1;
            const int st_ = jh_blockop_bidiag_step_range(op, b, t.p, t.s, 0.0, 1.0, 0, n, nullptr);      // (-alpha, 1) come from the device
            c.step_coef_dev = nullptr;
            c.step_done_dev = nullptr;
            c.step_skip_fold = 0;
            JH_TRY(st_);
            nparts_r = c.last_step_parts;
            rparts = c.part_dev;
        }
        const void *yv = cgls ? nullptr : t.y->data;
        const double *fold_n = fuse ? parts_n : nullptr;
        if (f64) hipLaunchKernelGGL((k_cg_xs<double>), dim3(grid), dim3(256), 0, c.stream, (double *)x->data, (double *)t.s->data, (const double *)t.p->data, (const double *)yv, ns_dom, t.st, parts_s, fold_n, nparts_n);
        else hipLaunchKernelGGL((k_cg_xs<float>), dim3(grid), dim3(256), 0, c.stream, (float *)x->data, (float *)t.s->data, (const float *)t.p->data, (const float *)yv, ns_dom, t.st, parts_s, fold_n, nparts_n);
        hipLaunchKernelGGL(k_cg_fold, dim3(1), dim3(256), 0, c.stream, (const double *)parts_s, (int64_t)grid, rparts, nparts_r, t.st, t.hist, slots, 2, on_device);
        JH_CHECK_HIP(hipGetLastError());
        return JH_OK;
    };
    double sums[2] = {0.0, 0.0};
    auto pull_sums = [&]() -> int {
        JH_CHECK_HIP(hipMemcpyAsync(sums, slots, sizeof(sums), hipMemcpyDeviceToHost, c.stream));
        JH_CHECK_HIP(hipStreamSynchronize(c.stream));
        return JH_OK;
    };
    // one host-driven iteration: the same kernels, the scalar updates applied HERE between them
    std::vector<double> hist_host(history ? 2 * (size_t)maxiter : 0);
    auto host_iteration = [&]() -> int {
        JH_TRY(half1(0));
        JH_TRY(pull_sums());
        cg_s1(&h, sums[0]);
        JH_TRY(push_state());
        if (h.done) return JH_OK;
        JH_TRY(half2(0));
        JH_TRY(pull_sums());
        cg_s2(&h, sums[0], sums[1], history ? hist_host.data() : nullptr);
        return push_state();
    };
    if (c.lsqr_graph == 0) {                                              // knob lsqr_graph = 0: host-driven, iteration by iteration
        while (!h.done) JH_TRY(host_iteration());
        if (history && h.itn > 0) memcpy(history, hist_host.data(), sizeof(double) * 2 * (size_t)h.itn);
        return finish();
    }
    // iteration 1 eagerly, the scalar updates on the device (workspaces get their size; the step kernel's shape is settled)
    struct Flags { int itn, istop, done; } fl{};
    auto read_flags = [&]() -> int {
        JH_CHECK_HIP(hipMemcpyAsync(&fl, &t.st->itn, sizeof(fl), hipMemcpyDeviceToHost, c.stream));
        JH_CHECK_HIP(hipStreamSynchronize(c.stream));
        return JH_OK;
    };
    fuse = !cgls;                                                         // (CGLS's step needs alpha before the vector update: its first fold stays a launch)
    JH_TRY(half1(1));
    JH_TRY(half2(1));
    JH_TRY(read_flags());
    int64_t replays = 0;
    if (!fl.done) {
        if (cgls && !(nparts_r > 0 && nparts_r <= 8192)) return jh_fail(JH_ERR_STATE, "device-resident CGLS: the step left %lld partial sums (expected 1..8192)", (long long)nparts_r);
        const uint64_t gen = c.buf_gen;
        // EIGHT iterations per graph (a finished solve replays as no-ops): one hipGraphLaunch costs the host 10-16 us, about what a whole
        // iteration of a 64 x 64^3 operator takes on the device
        const int per_graph = maxiter < 8 ? maxiter : 8;
        JH_CHECK_HIP(hipStreamBeginCapture(c.stream, hipStreamCaptureModeRelaxed));
        int st_ = JH_OK;
        for (int k = 0; k < per_graph && st_ == JH_OK; k++) {
            st_ = half1(1);
            if (st_ == JH_OK) st_ = half2(1);
        }
        hipError_t e = hipStreamEndCapture(c.stream, &t.graph);
        if (st_ != JH_OK) return st_;
        JH_CHECK_HIP(e);
        JH_REQUIRE(gen == c.buf_gen, "device-resident CG: a workspace was reallocated during capture");
        JH_CHECK_HIP(hipGraphInstantiate(&t.exec, t.graph, nullptr, nullptr, 0));
        while (!fl.done) {                                                // two graphs between two looks at the flags
            for (int k = 0; k < 2; k++) JH_CHECK_HIP(hipGraphLaunch(t.exec, c.stream));
            replays += 2;
            JH_TRY(read_flags());
        }
    }
    c.last_cg_graph = replays;
    JH_CHECK_HIP(hipMemcpyAsync(&h, t.st, sizeof(h), hipMemcpyDeviceToHost, c.stream));
    JH_CHECK_HIP(hipStreamSynchronize(c.stream));
    if (history && h.itn > 0) {
        JH_CHECK_HIP(hipMemcpyAsync(history, t.hist, sizeof(double) * 2 * (size_t)h.itn, hipMemcpyDeviceToHost, c.stream));
        JH_CHECK_HIP(hipStreamSynchronize(c.stream));
    }
    return finish();
}

extern "C" int jh_cgls_solve(const jh_blockop *op, jh_bvec *u, jh_bvec *x, int use_x0, double damp, double atol, double btol, int maxiter,
                             int force_maxiter, jh_lsqr_result *res, double *history)
{
    bool took = false;
    JH_TRY(cg_dev_impl(op, u, x, use_x0, damp, atol, btol, maxiter, force_maxiter, res, history, true, &took));   // small operators: recurrences on the device
    if (took) return JH_OK;
    return cgls_impl(1, &op, &u, &x, use_x0, damp, atol, btol, maxiter, force_maxiter, res, history, Exch::none, nullptr, true);
}

extern "C" int jh_cgls_solve_partitioned(const jh_blockop *op, jh_bvec *u, jh_bvec *x, int use_x0, double damp, double atol, double btol,
                                         int maxiter, int force_maxiter, jh_lsqr_result *res, double *history)
{
    Exch ex = Exch::none;
    JH_TRY(partitioned_exchange("jh_cgls_solve", op, u, x, &ex));
    return cgls_impl(1, &op, &u, &x, use_x0, damp, atol, btol, maxiter, force_maxiter, res, history, ex);
}

extern "C" int jh_cgls_solve_team(int n, const jh_blockop *const *ops, jh_bvec *const *us, jh_bvec *const *xs, int use_x0, double damp, double atol,
                                  double btol, int maxiter, int force_maxiter, jh_lsqr_result *res, double *history)
{
    JH_TRY(team_members_ok("jh_cgls_solve", n, ops, us, xs));
    return cgls_impl(n, ops, us, xs, use_x0, damp, atol, btol, maxiter, force_maxiter, res, history, Exch::team);
}

// ------------------------------------------------------------------ CG on the normal equations through the fused A'A (round 3) -------------
// BASELINE.json configs[2] is "JetComposite A' o A normal-equations matvec ... (chain fusion + reductions)": this is the solver that
// matvec is for.  Conjugate gradients applied to (A'A + damp^2 I) x = A'b with the fused normal operator (jh_blockop_normal_mul reads
// the coefficients ONCE and never forms a range-sized intermediate): after ONE adjoint pass for A'b an iteration moves N n s bytes --
// a third of LSQR's one-pass iteration, a quarter of CGLS's -- plus domain-sized vectors; the range vector b is read once and never
// written.  In exact arithmetic the iterates are CGLS's / LSQR's; in floating point the residual s = A'r lives in the DOMAIN and is
// updated by recurrence (s -= alpha (A'A + damp^2) p) instead of being recomputed from r, the textbook weakness of "CGNR done
// naively" (Bjorck 1996, section 7.4): the attainable accuracy degrades with cond(A)^2 where CGLS / LSQR keep cond(A).  For the
// well-conditioned operators of the benchmark (every column sums N squared coefficients) it reaches the same x; ||r|| is tracked by
// its own recurrence ||r_k||^2 = ||r_{k-1}||^2 - alpha_k gamma_{k-1} (exact for CG), so no pass over the range is needed for it.
// Partitioned: every shard's A_k'A_k p in 4 element ranges (jh_blockop_normal_mul_range), each range all-reduced on the exchange stream
// under the next range's kernel; the scalars come from the replicated vectors, so the exchange of y is the only collective.
static int cgnr_impl(const int M, const jh_blockop *const *ops, jh_bvec *const *bs, jh_bvec *const *xs, int use_x0, double damp, double atol,
                     double btol, int maxiter, int force_maxiter, jh_lsqr_result *res, double *history, const Exch ex,
                     const jh_chain *ch = nullptr)
{
    Shards sh("jh_cgnr_solve", M, ops, bs, xs, ex);
    // a chain; a tall operator of two rows or more; (round 6) one unpartitioned shard may also be an N x (2 .. 4) grid of equal diagonals -- its fused A'A is
    // jh_grid_normal.hip; the loop below only ever calls jh_blockop_mul_adj and jh_blockop_normal_mul on whole vectors there
    JH_TRY(sh.init(res, maxiter, [&](int k) {
        if (ch || (M == 1 && ex == Exch::none && jhb::grid_normal_ok(ops[k], xs[k]->data, xs[k]->data))) return true;
        return sh.tall(k) && ops[k]->nrow >= 2;
    }, "a tall (>= 2 rows) operator of equal elementwise rows (or, unpartitioned, an N x (2 .. 4) grid of equal diagonals)"));
    std::vector<Passes> pass = passes_of(sh, ch);
    std::vector<DomVecs<3>> t((size_t)M);
    for (int k = 0; k < M; k++) {
        JH_TRY(sh.use(k));
        JH_TRY(t[k].create(sh.n, sh.dtype));
    }
    *res = jh_lsqr_result{};
    auto allreduce = [&](int which) { return sh.grouped([&](int k) { return jh_comm_allreduce_sum(t[k][which]); }); };   // every member's domain vector summed over the shards

    // ||b||, s = A'b
    double s2 = 0.0;
    JH_TRY(start_norm_b(sh, use_x0, &s2));
    const double bnorm = std::sqrt(s2);
    for (int k = 0; k < M; k++) JH_TRY(pass[k].adjoint(t[k][S], bs[k]));
    JH_TRY(allreduce(S));
    double rr = s2;                                                       // ||b - A x||^2, by recurrence
    if (use_x0) {                                                         // s = A'b - (A'A + damp^2) x0 ;  ||r0||^2 = ||b||^2 - 2 Re<x0, A'b> + <x0, A'A x0>
        for (int k = 0; k < M; k++) JH_TRY(pass[k].normal(t[k][Y], xs[k]));
        JH_TRY(allreduce(Y));
        double xb = 0.0, xax = 0.0, im = 0.0;
        JH_TRY(jh_dot(xs[0], t[0][S], &xb, &im));
        JH_TRY(jh_dot(xs[0], t[0][Y], &xax, &im));
        rr = s2 - 2.0 * xb + xax;
        if (damp != 0.0) {                                                // the functional CG decreases is ||r||^2 + damp^2 ||x||^2
            double x0n = 0.0;
            JH_TRY(jh_norm(xs[0], 2.0, &x0n));
            rr += damp * damp * x0n * x0n;
        }
        for (int k = 0; k < M; k++) {
            JH_TRY(lincomb2(t[k][S], 1.0, t[k][S], -1.0, t[k][Y]));
            if (damp != 0.0) JH_TRY(lincomb2(t[k][S], 1.0, t[k][S], -damp * damp, xs[k]));
        }
    }
    double nrm = 0.0;
    JH_TRY(jh_norm(t[0][S], 2.0, &nrm));
    double gamma = nrm * nrm;
    const double gamma0 = gamma;
    for (int k = 0; k < M; k++) JH_TRY(jh_copy(t[k][P], t[k][S]));
    int itn = 0, istop = 0;
    // y = sum over the shards of A_k'A_k p.  Partitioned: in 4 element ranges -- the all-reduce of a finished range runs on the exchange
    // stream while the kernel of the next range computes; the library streams then wait for the exchange (no host synchronisation)
    auto normal_all = [&]() -> int {
        if (ex == Exch::none) return pass[0].normal(t[0][Y], t[0][P]);
        JH_TRY(sh.for_ranges([&](int64_t lo, int64_t cnt) -> int {
            for (int k = 0; k < M; k++) JH_TRY(jh_blockop_normal_mul_range(ops[k], t[k][Y], t[k][P], lo, cnt));
            return sh.grouped([&](int k) { return jh_comm_allreduce_sum_range(t[k][Y], lo, cnt); });
        }));
        for (int k = 0; k < M; k++) { JH_TRY(sh.use(k)); JH_TRY(jh_comm_join()); }
        return JH_OK;
    };
    if (gamma > 0) {
        while (itn < maxiter) {
            itn++;
            JH_TRY(normal_all());                                         // the ONE pass over the operator
            if (damp != 0.0)
                for (int k = 0; k < M; k++) JH_TRY(lincomb2(t[k][Y], 1.0, t[k][Y], damp * damp, t[k][P]));
            double delta = 0.0, im = 0.0;
            JH_TRY(jh_dot(t[0][P], t[0][Y], &delta, &im));                  // replicas are identical: member 0 speaks for all
            if (!(delta > 0) || !std::isfinite(delta)) {
                istop = 6;
                itn--;
                break;
            }
            const double alpha = gamma / delta;
            for (int k = 0; k < M; k++) {
                JH_TRY(lincomb2(xs[k], 1.0, xs[k], alpha, t[k][P]));      // x += alpha p
                JH_TRY(lincomb2(t[k][S], 1.0, t[k][S], -alpha, t[k][Y]));   // s -= alpha (A'A + damp^2) p
            }
            rr -= alpha * gamma;                                          // ||r||^2 (+ damp^2 ||x||^2 when damped: the functional's value)
            if (rr < 0) rr = 0;
            JH_TRY(jh_norm(t[0][S], 2.0, &nrm));
            const double gamma_new = nrm * nrm;
            const double bk = gamma_new / gamma;
            for (int k = 0; k < M; k++) JH_TRY(lincomb2(t[k][P], 1.0, t[k][S], bk, t[k][P]));
            gamma = gamma_new;
            const double rnorm = std::sqrt(rr), arnorm = std::sqrt(gamma);
            if (history) { history[2 * (itn - 1)] = rnorm; history[2 * (itn - 1) + 1] = arnorm; }
            if (itn >= maxiter) istop = 7;
            if (arnorm <= atol * std::sqrt(gamma0)) istop = 2;
            if (rnorm <= btol * bnorm) istop = 1;
            if (istop && !(force_maxiter && itn < maxiter && gamma > 0)) break;
        }
    }
    double xnorm = 0.0;
    JH_TRY(jh_norm(xs[0], 2.0, &xnorm));
    res->istop = istop;
    res->itn = itn;
    res->r2norm = std::sqrt(rr);                                          // sqrt(||r||^2 + damp^2 ||x||^2): what the recurrence tracks
    const double r1sq = rr - damp * damp * xnorm * xnorm;
    res->r1norm = std::sqrt(r1sq > 0 ? r1sq : 0.0);
    res->anorm = 0.0;
    res->acond = 0.0;
    res->arnorm = std::sqrt(gamma);
    res->xnorm = xnorm;
    return sh.sync_all();
}

extern "C" int jh_cgnr_solve(const jh_blockop *op, jh_bvec *b, jh_bvec *x, int use_x0, double damp, double atol, double btol, int maxiter,
                             int force_maxiter, jh_lsqr_result *res, double *history)
{
    bool took = false;
    JH_TRY(cg_dev_impl(op, b, x, use_x0, damp, atol, btol, maxiter, force_maxiter, res, history, false, &took));  // small operators: recurrences on the device
    if (took) return JH_OK;
    return cgnr_impl(1, &op, &b, &x, use_x0, damp, atol, btol, maxiter, force_maxiter, res, history, Exch::none);
}

extern "C" int jh_cgnr_solve_partitioned(const jh_blockop *op, jh_bvec *b, jh_bvec *x, int use_x0, double damp, double atol, double btol,
                                         int maxiter, int force_maxiter, jh_lsqr_result *res, double *history)
{
    Exch ex = Exch::none;
    JH_TRY(partitioned_exchange("jh_cgnr_solve", op, b, x, &ex));
    return cgnr_impl(1, &op, &b, &x, use_x0, damp, atol, btol, maxiter, force_maxiter, res, history, ex);
}

extern "C" int jh_cgnr_solve_team(int n, const jh_blockop *const *ops, jh_bvec *const *bs, jh_bvec *const *xs, int use_x0, double damp, double atol,
                                  double btol, int maxiter, int force_maxiter, jh_lsqr_result *res, double *history)
{
    JH_TRY(team_members_ok("jh_cgnr_solve", n, ops, bs, xs));
    return cgnr_impl(n, ops, bs, xs, use_x0, damp, atol, btol, maxiter, force_maxiter, res, history, Exch::team);
}

// ------------------------------------------------------------------ the solvers on a FORWARD chain (weighted least squares) ---------------
// lsqr(W o A o M, b) and its siblings (docs/src/index.md:235-246): the loops above with the four passes of the chain (Passes), one GPU, host-driven
// at every size.  Declined (JH_ERR_UNSUPPORTED) before anything is touched where the step is: the caller keeps its generic loop.
static int chain_solver_args(const jh_chain *fwd, const jh_bvec *u, const jh_bvec *x, const jh_blockop **op, const char *fn, bool needs_step = true)
{
    JH_REQUIRE(fwd && u && x, "%s: null argument", fn);
    JH_TRY(jhb::chain_solver_ok(fwd, u, x, op, needs_step));
    JH_TRY(jh_enter(*op, u, x));
    return JH_OK;
}

extern "C" int jh_lsqr_solve_chain(const jh_chain *fwd, jh_bvec *u, jh_bvec *x, int use_x0, double damp, double atol, double btol, double conlim,
                                   int maxiter, int force_maxiter, jh_lsqr_result *res, double *history)
{
    const jh_blockop *op = nullptr;
    JH_TRY(chain_solver_args(fwd, u, x, &op, "jh_lsqr_solve_chain"));
    return lsqr_impl(1, &op, &u, &x, use_x0, damp, atol, btol, conlim, maxiter, force_maxiter, res, history, Exch::none, fwd);
}

extern "C" int jh_cgls_solve_chain(const jh_chain *fwd, jh_bvec *u, jh_bvec *x, int use_x0, double damp, double atol, double btol, int maxiter,
                                   int force_maxiter, jh_lsqr_result *res, double *history)
{
    const jh_blockop *op = nullptr;
    JH_TRY(chain_solver_args(fwd, u, x, &op, "jh_cgls_solve_chain"));
    return cgls_impl(1, &op, &u, &x, use_x0, damp, atol, btol, maxiter, force_maxiter, res, history, Exch::none, fwd);
}

extern "C" int jh_cgnr_solve_chain(const jh_chain *fwd, jh_bvec *b, jh_bvec *x, int use_x0, double damp, double atol, double btol, int maxiter,
                                   int force_maxiter, jh_lsqr_result *res, double *history)
{
    const jh_blockop *op = nullptr;
    JH_TRY(chain_solver_args(fwd, b, x, &op, "jh_cgnr_solve_chain", false));   // (the ADJOINT and NORMAL programs only: a grid chain takes it too)
    return cgnr_impl(1, &op, &b, &x, use_x0, damp, atol, btol, maxiter, force_maxiter, res, history, Exch::none, fwd);
}
