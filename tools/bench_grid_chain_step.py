#!/usr/bin/env python3
"""The one-pass Golub-Kahan step of a FORWARD chain W o A through an N x K grid (jh_grid_chain_step.hip, knob grid_chain_step = 1) and the native
LSQR / CGLS loops on it, against the route it replaces (knob 0, the default: the step is declined, so LSQR and CGLS run the FORWARD grid chain into
a range temporary, a range lincomb and norm, and the ADJOINT grid chain), alternating the two in one process.

    python tools/bench_grid_chain_step.py [nrow ncol edge [dtype]]        default: the issue's set of cases

Algorithmic bytes per step (s = element size, N x K blocks of n elements, one weight stream): the one-pass step (N K + 3 N + 2 K) n s (coefficients,
weights, u read and written, v read, w written); the two-pass route (2 N K + 8 N + 2 K) n s (FORWARD N K + 2 N + K, lincomb 3 N, norm N, ADJOINT
N K + 2 N + K).  Output lines: "ALGO <kernel regex> <bytes>" for tools/prof_any.sh, then ms per step and per LSQR / CGLS iteration, and the relative
difference of the two routes' solutions."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import jets_jl_amd as J
from jets_jl_amd import chains
from jets_jl_amd.arrays import lincomb_, norm

PEAK = 8.0e12
J.init(0)


def step_bytes(N, K, n, s):
    return (N * K + 3 * N + 2 * K) * n * s, (2 * N * K + 8 * N + 2 * K) * n * s


def timed(fn, reps):
    fn()
    J.synchronize()
    e0 = J.Event().record()
    for _ in range(reps):
        fn()
    e1 = J.Event().record()
    return e0.elapsed_ms(e1) / reps


def knob(v):
    J.tune(grid_chain_step=v)


def ab(fn, reps, rounds=3):
    """(one-pass step, two-pass route), alternating: the best of `rounds` each"""
    f, u = [], []
    for _ in range(rounds):
        knob(1)
        try:
            f.append(timed(fn, reps))
        finally:
            knob(0)
        u.append(timed(fn, reps))
    return min(f), min(u)


def weighted_grid(nrow, ncol, edge, dt):
    blk = J.JetSpace(dt, edge, edge, edge)
    coeff = J.rand(J.JetBSpace([blk] * (nrow * ncol)), seed=1, stream=0)
    A = J.blockop([[J.JopDiagonal(coeff.arrays[i * ncol + k]) for k in range(ncol)] for i in range(nrow)])
    w = J.rand(J.range(A), seed=5, stream=0)
    return A, J.compose(J.JopDiagonal(w), A), blk.length()


def case(nrow, ncol, edge, dt=np.float32, iters=10):
    A, L, n = weighted_grid(nrow, ncol, edge, dt)
    s = np.dtype(dt).itemsize
    new_b, old_b = step_bytes(nrow, ncol, n, s)
    reps = max(3, int(4.0e10 / new_b))
    print(f"# W o A, {nrow} x {ncol} of {edge}^3 {np.dtype(dt).name}: {nrow * ncol * n * s / 2**30:.1f} GiB of coefficients, {reps} repetitions", flush=True)
    cty = {np.float32: "float, 1, 4", np.float64: "double, 1, 2"}.get(dt)
    if cty:
        print(f"ALGO k_grid_chain_step<{cty}, {ncol}, \\d, \\w+, 1, true>".replace(" ", "\\s") + f" {new_b}", flush=True)
    sc = chains.SolverChains(L)
    assert sc.fwd is not None and sc.fwd.grid, "W o A did not plan to one FORWARD grid chain"
    u = J.rand(J.range(L), seed=3, stream=0)
    v = J.rand(J.domain(L), seed=2, stream=0)
    w = J.zeros(J.domain(L))
    t = None

    def step():
        nonlocal t
        if J.tune_get("grid_chain_step"):
            assert sc.step(u, v, w, 1.0, -0.5) is not None
            return
        if t is None:
            t = J.zeros(J.range(L))
        J.mul_(t, L, v)                                          # what lsqr._Engine._fwd_local does on a composite, then the adjoint half
        lincomb_(u, [1.0, -0.5], [t, u])
        float(norm(u))
        J.mul_(w, L.H, u)

    ms_f, ms_u = ab(step, reps)
    t = None
    print(f"{'step':8s} one pass {ms_f:9.3f} ms  {new_b / 1e9:8.2f} GB  {new_b / (ms_f * 1e-3) / 1e12:5.2f} TB/s  {100 * new_b / (ms_f * 1e-3) / PEAK:5.1f} % of 8 TB/s   "
          f"two passes {ms_u:9.3f} ms  {old_b / 1e9:8.2f} GB  {old_b / (ms_u * 1e-3) / 1e12:5.2f} TB/s   {ms_u / ms_f:5.2f}x", flush=True)
    del u, v, w
    sc.close()
    b = J.rand(J.range(L), seed=9, stream=0)
    for name in ("lsqr", "cgls"):
        fn = getattr(J, name)
        f, o, xs = [], [], {}
        for _ in range(2):
            for k in (1, 0):
                knob(k)
                try:
                    g0 = chains.STATS["chain_solve_calls"]
                    J.synchronize()
                    e0 = J.Event().record()
                    r = fn(L, b, maxiter=iters, atol=0.0, btol=0.0, force_maxiter=True)
                    e1 = J.Event().record()
                    assert (chains.STATS["chain_solve_calls"] > g0) == (k == 1), "the route is not the one the knob asks for"
                    (f if k else o).append(e0.elapsed_ms(e1) / iters)
                    xs[k] = r.x.to_numpy().ravel(order="F").astype(np.float64)
                    del r
                finally:
                    knob(0)
        diff = np.linalg.norm(xs[1] - xs[0]) / np.linalg.norm(xs[0])
        print(f"{name.upper():8s} one pass {min(f):9.3f} ms/iteration   two passes {min(o):9.3f} ms/iteration   {min(o) / min(f):5.2f}x   "
              f"|x_new - x_old| / |x_old| = {diff:.2e}", flush=True)
    J.close(A)


if len(sys.argv) > 3:
    dt = {"f32": np.float32, "f64": np.float64, "c32": np.complex64, "c64": np.complex128}[sys.argv[4] if len(sys.argv) > 4 else "f32"]
    case(int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), dt)
else:
    case(64, 4, 256)
    case(128, 2, 256)
    case(64, 3, 256)
    case(4096, 3, 64)
    case(64, 4, 255)
