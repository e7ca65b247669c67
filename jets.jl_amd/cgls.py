"""CGLS over the Jets operator API ("LSQR/CGLS solver driver").

Conjugate gradients on the normal equations (Hestenes & Stiefel 1952; Bjorck 1996, algorithm 7.4.1): min ||A x - b||^2
(+ damp^2 ||x||^2).  Like LSQR it has no counterpart inside Jets.jl (src/Jets.jl:1143-1152 points its users at
IterativeSolvers.jl, un-vendored): the published recurrence, checked against the fp64 CPU CGLS of oracle/cgls_ref.py.

For a device-native tall block operator the whole loop runs behind the C ABI (jh_cgls_solve / _partitioned / _team): TWO
passes per iteration and no range-sized temporary -- ||A p||^2 = <p, A'A p> through the fused normal operator (N n s bytes),
then r <- r - alpha A p, ||r||^2 and A'r in one pass of the Golub-Kahan step kernel (3 N n s).  Any other operator runs the
textbook loop (q = A p kept in a range vector) over the same engines as LSQR: the two fused halves where they exist
(jh_blockop_mul_axpby / jh_blockop_mul_adj_axpby), plain mul! otherwise; row-partitioned and team operators included.  A WEIGHTED shard or team
(L = W o A, ...) under an exchange takes the two-pass form here too (cgls_core, `step_cgls`): <p, L'L p> through the ranged NORMAL chain, then the
ranged one-pass chain step (jh_chain_bidiag_step_range) -- no range-sized temporary.
"""
from __future__ import annotations

import builtins
import math

from .lsqr import LsqrResult, _engine_for, _native_solve

__all__ = ["cgls", "cgls_core", "cgnr", "cgnr_core"]


def cgls(A, b, x0=None, damp: float = 0.0, atol: float = 1e-6, btol: float = 1e-6, maxiter: int = 100, overwrite_b: bool = False,
         force_maxiter: bool = False) -> LsqrResult:
    """x, info = cgls(A, b).  `b` lives in range(A), the result in domain(A); `A` may be a rowpart.RowPartitionedOp (b = this
    rank's rows, every rank gets the same x) or a rowpart.TeamOp (b, x: TeamVec).  istop: 1 ||r|| <= btol ||b||, 2 ||A'r - damp^2 x||
    <= atol times its starting value, 6 breakdown, 7 maxiter.  The record is LSQR's (r1norm = ||r||, arnorm = ||A'r - damp^2 x||,
    history = (itn, ||r||, ||A'r - damp^2 x||) per iteration; anorm = acond = 0).  `overwrite_b=True`: b's storage becomes r."""
    eng, b, x0 = _engine_for(A, b, x0)
    res = _native_solve(eng, "cgls", b, x0, (damp, atol, btol), maxiter, force_maxiter, copy_b=not overwrite_b)
    return res if res is not None else cgls_core(eng, b, x0, damp, atol, btol, maxiter, overwrite_b, force_maxiter)


def cgls_core(eng, b, x0, damp, atol, btol, maxiter, overwrite_b=False, force_maxiter=False) -> LsqrResult:
    """The textbook loop on an engine (lsqr._Engine's interface: zeros_dom / zeros_rng / copy / lincomb / norm_dom / norm_rng and the
    two half-iterations fwd(u, v, alpha, beta) -> ||alpha A v + beta u||, adj(v, u, alpha, beta) -> ||alpha A'u + beta v||)."""
    x = eng.zeros_dom() if x0 is None else eng.copy(eng.zeros_dom(), x0)
    r = b if overwrite_b else eng.copy(eng.zeros_rng(), b)
    bnorm = eng.norm_rng(b)
    rnorm = eng.fwd(r, x, -1.0, 1.0) if x0 is not None else bnorm          # r = b - A x0
    # an engine with a one-pass step AND a `normal` hook that asks for it (`step_cgls`: a weighted shard or team, lsqr._ShardEngine / _TeamEngine; one GPU: a weighted grid with the knob grid_chain_step = 1)
    # runs the two passes of jh_lsqr.hip's cgls_impl: delta = <p, A'A p> through the hook, then r <- r - alpha A p, ||r|| and A'r in one step --
    # no q.  Should the step decline (before anything is touched), the textbook passes take over from that iteration on.
    two_pass = bool(getattr(eng, "step_cgls", False))
    s, p = eng.zeros_dom(), eng.zeros_dom()
    q = None if two_pass else eng.zeros_rng()
    y = eng.zeros_dom() if two_pass else None
    eng.adj(s, r, 1.0, 0.0)                                                 # s = A'r
    if damp:
        eng.lincomb(s, [1.0, -damp * damp], [s, x])
    gamma = eng.norm_dom(s) ** 2
    gamma0 = gamma
    eng.copy(p, s)
    history, itn, istop = [], 0, 0
    if gamma > 0:
        while itn < maxiter:
            itn += 1
            if two_pass:
                pap = getattr(eng, "normal_cgls", eng.normal)(y, p)         # <p, A'A p> in one pass (normal_cgls: a hook that exchanges the scalar only -- y is not used further)
                if pap is None:                                             # (the hook's kernel was declined before anything was touched: the textbook passes)
                    two_pass, q = False, eng.zeros_rng()
                    pap = eng.fwd(q, p, 1.0, 0.0) ** 2
                delta = pap + (damp * eng.norm_dom(p)) ** 2
            else:
                qn = eng.fwd(q, p, 1.0, 0.0)                                 # q = A p, ||q||
                delta = qn * qn + (damp * eng.norm_dom(p)) ** 2
            if not (delta > 0 and math.isfinite(delta)):
                istop, itn = 6, itn - 1
                break
            alpha = gamma / delta
            eng.lincomb(x, [1.0, alpha], [x, p])
            fused = eng.step(r, p, -alpha, 1.0) if two_pass else None       # r <- r - alpha A p ; ||r|| ; A'r
            if fused is not None:
                rnorm = fused[0]
                eng.copy(s, fused[1])
            else:
                if two_pass:
                    two_pass, q = False, eng.zeros_rng()
                    eng.fwd(q, p, 1.0, 0.0)
                eng.lincomb(r, [1.0, -alpha], [r, q])
                rnorm = eng.norm_rng(r)
                eng.adj(s, r, 1.0, 0.0)                                     # s = A'r - damp^2 x
            if damp:
                eng.lincomb(s, [1.0, -damp * damp], [s, x])
            gamma_new = eng.norm_dom(s) ** 2
            eng.lincomb(p, [1.0, gamma_new / gamma], [s, p])
            gamma = gamma_new
            arnorm = math.sqrt(gamma)
            history.append((itn, rnorm, arnorm))
            if itn >= maxiter:
                istop = 7
            if arnorm <= atol * math.sqrt(gamma0):
                istop = 2
            if rnorm <= btol * bnorm:
                istop = 1
            if istop and not (force_maxiter and itn < maxiter and gamma > 0):
                break
    xnorm = eng.norm_dom(x)
    return LsqrResult(x, istop, itn, rnorm, math.sqrt(rnorm ** 2 + (damp * xnorm) ** 2), 0.0, 0.0, math.sqrt(gamma), xnorm, history)


# ------------------------------------------------------------------ CG on the normal equations through the fused A'A
def cgnr(A, b, x0=None, damp: float = 0.0, atol: float = 1e-6, btol: float = 1e-6, maxiter: int = 100, force_maxiter: bool = False) -> LsqrResult:
    """Conjugate gradients on (A'A + damp^2 I) x = A'b with the normal operator applied as ONE fused pass (JetComposite (A', A),
    src/Jets.jl:530-534 -> jh_blockop_normal_mul): after one adjoint pass for A'b an iteration reads the coefficients once
    (N n s bytes, a third of the LSQR iteration) and works on domain-sized vectors; b is read once and never written; ||r|| follows
    the exact CG recurrence.  Same iterates as cgls / lsqr in exact arithmetic; the attainable accuracy goes with cond(A)^2 (the
    residual A'r is updated by recurrence in the domain), so: well-conditioned operators, throughput.  A device-native tall block
    operator runs behind the C ABI (jh_cgnr_solve / _partitioned / _team); anything else applies A then A' through the engines.
    The record: r2norm = sqrt(||r||^2 + damp^2 ||x||^2) from the recurrence, r1norm = ||r|| derived from it, arnorm = ||A'r - damp^2 x||."""
    eng, b, x0 = _engine_for(A, b, x0)
    res = _native_solve(eng, "cgnr", b, x0, (damp, atol, btol), maxiter, force_maxiter, copy_b=False)     # (b is read, never written)
    return res if res is not None else cgnr_core(eng, b, x0, damp, atol, btol, maxiter, force_maxiter)


def cgnr_core(eng, b, x0, damp, atol, btol, maxiter, force_maxiter=False) -> LsqrResult:
    """The same recurrences on an engine: the normal operator as A then A' (two passes and a range-sized temporary -- operators without
    the fused kernel).  An engine with a `normal(y, p)` hook (y = A'A p in one pass, returns <p, A'A p> taken on the replicated domain vector:
    a weighted row-partitioned shard's NORMAL chain, lsqr._ShardEngine) applies the normal operator through it instead, with no range vector."""
    normal = getattr(eng, "normal", None)
    x = eng.zeros_dom() if x0 is None else eng.copy(eng.zeros_dom(), x0)
    bnorm = eng.norm_rng(b)
    s, p, y = eng.zeros_dom(), eng.zeros_dom(), eng.zeros_dom()
    q = eng.zeros_rng() if normal is None else None
    eng.adj(s, b, 1.0, 0.0)                                                 # s = A'b
    phi = bnorm * bnorm                                                     # ||r||^2 + damp^2 ||x||^2, by recurrence
    if x0 is not None:
        if normal is None:
            qn = eng.fwd(q, x, 1.0, 0.0)                                     # A x0
            eng.adj(y, q, 1.0, 0.0)                                         # A'A x0
            xax = qn * qn
        else:
            xax = normal(y, x)                                              # A'A x0, <x0, A'A x0>
        from .arrays import dot

        xb = dot(x[0], s[0]) if hasattr(x, "members") else dot(x, s)
        phi = phi - 2.0 * float(getattr(xb, "real", xb)) + xax + (damp * eng.norm_dom(x)) ** 2
        eng.lincomb(s, [1.0, -1.0], [s, y])
        if damp:
            eng.lincomb(s, [1.0, -damp * damp], [s, x])
    gamma = eng.norm_dom(s) ** 2
    gamma0 = gamma
    eng.copy(p, s)
    history, itn, istop = [], 0, 0
    if gamma > 0:
        while itn < maxiter:
            itn += 1
            if normal is None:
                qn = eng.fwd(q, p, 1.0, 0.0)                                 # q = A p ; <p, A'A p> = ||q||^2
                eng.adj(y, q, 1.0, 0.0)                                     # y = A'A p
                delta = qn * qn + (damp * eng.norm_dom(p)) ** 2
            else:
                delta = normal(y, p) + (damp * eng.norm_dom(p)) ** 2        # y = A'A p in one pass ; <p, y>
            if damp:
                eng.lincomb(y, [1.0, damp * damp], [y, p])
            if not (delta > 0 and math.isfinite(delta)):
                istop, itn = 6, itn - 1
                break
            alpha = gamma / delta
            eng.lincomb(x, [1.0, alpha], [x, p])
            eng.lincomb(s, [1.0, -alpha], [s, y])
            phi = builtins.max(phi - alpha * gamma, 0.0)
            gamma_new = eng.norm_dom(s) ** 2
            eng.lincomb(p, [1.0, gamma_new / gamma], [s, p])
            gamma = gamma_new
            rnorm, arnorm = math.sqrt(phi), math.sqrt(gamma)
            history.append((itn, rnorm, arnorm))
            if itn >= maxiter:
                istop = 7
            if arnorm <= atol * math.sqrt(gamma0):
                istop = 2
            if rnorm <= btol * bnorm:
                istop = 1
            if istop and not (force_maxiter and itn < maxiter and gamma > 0):
                break
    xnorm = eng.norm_dom(x)
    r1sq = phi - (damp * xnorm) ** 2
    return LsqrResult(x, istop, itn, math.sqrt(builtins.max(r1sq, 0.0)), math.sqrt(phi), 0.0, 0.0, math.sqrt(gamma), xnorm, history)
