#!/usr/bin/env python3
"""Fused chains through an N x K grid against the stage-by-stage composite (jets.jl_amd/chains.py, jh_grid_chain.hip), alternating the two in one
process (chains.ENABLED).

    python tools/bench_grid_chains.py [nrow ncol edge [dtype]]        default: the issue's set of cases

Algorithmic bytes (s = element size, N x K blocks of n elements):  A' o W o A: N K n s + N n s + 2 K n s;  (W o A)': N K n s + 2 N n s + K n s;
W o A: N K n s + 2 N n s + K n s;  M' o A' o W o A o M: N K n s + N n s + 4 K n s."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import jets_jl_amd as J
from jets_jl_amd import chains

PEAK = 8.0e12
J.init(0)
for kv in os.environ.get("JETS_TUNE", "").split(","):          # e.g. JETS_TUNE=nt=0 (A/B of the load policy)
    if "=" in kv:
        J.tune(**{kv.split("=")[0]: int(kv.split("=")[1])})


def timed(fn, reps):
    fn()
    J.synchronize()
    e0 = J.Event().record()
    for _ in range(reps):
        fn()
    e1 = J.Event().record()
    return e0.elapsed_ms(e1) / reps


def ab(fn, reps, rounds=3):
    """fused / stage-by-stage, alternating: the best of `rounds` each"""
    f, u = [], []
    for _ in range(rounds):
        chains.ENABLED[0] = True
        f.append(timed(fn, reps))
        chains.ENABLED[0] = False
        try:
            u.append(timed(fn, max(1, reps // 2)))
        finally:
            chains.ENABLED[0] = True
    return min(f), min(u)


def grid(nrow, ncol, edge, dt, lam_rows=False):
    blk = J.JetSpace(dt, edge, edge, edge)
    rows = []
    for i in range(nrow):
        rows.append([J.JopDiagonal(J.rand(blk, seed=1, stream=100 * i + k)) for k in range(ncol)])
    if lam_rows:
        for r in range(ncol):
            lam = J.JopLn(dom=blk, rng=blk, df=J.constdiag_df, df_adj=J.constdiag_df_adj, s={"a": 0.1})
            rows.append([lam if k == r else J.JopZeroBlock(blk, blk) for k in range(ncol)])
    return J.blockop(rows), blk.length()


def case(nrow, ncol, edge, dt=np.float32, lam_rows=False, solvers=False):
    A, n = grid(nrow, ncol, edge, dt, lam_rows)
    N = nrow + (ncol if lam_rows else 0)
    s = np.dtype(dt).itemsize
    W = J.JopDiagonal(J.rand(J.range(A), seed=5, stream=0))
    M = J.JopDiagonal(J.rand(J.domain(A), seed=6, stream=0))
    m = J.rand(J.domain(A), seed=2, stream=0)
    y = J.zeros(J.domain(A))
    d = J.rand(J.range(A), seed=3, stream=0)
    NKn, Nn, Kn = N * ncol * n * s, N * n * s, ncol * n * s
    reps = max(3, int(1.0e11 / NKn))
    print(f"# {N} x {ncol} of {edge}^3 {np.dtype(dt).name}{' (incl. lam I rows)' if lam_rows else ''}: {NKn / 2**30:.1f} GiB of coefficients, {reps} repetitions", flush=True)
    # ("ALGO <kernel regex> <bytes>": the algorithmic bytes of each grid chain kernel for tools/prof_any.sh; one range weight, NW = 1)
    cty = {np.float32: "float, 1, 4", np.float64: "double, 1, 2"}.get(dt)
    if cty and not lam_rows:
        for mode, nb in ((2, NKn + Nn + 2 * Kn), (1, NKn + 2 * Nn + Kn), (0, NKn + 2 * Nn + Kn)):
            rx = f"k_grid_chain<{cty}, {ncol}, 2, \\w+, {mode}, 1>".replace(" ", "\\s")           # (no blanks: the line is split on them)
            print(f"ALGO {rx} {nb}", flush=True)
    for tag, op, out, x, nbytes in (
        ("A' o W o A", J.compose(J.compose(A.H, W), A), y, m, NKn + Nn + 2 * Kn),
        ("(W o A)'", J.compose(W, A).H, y, d, NKn + 2 * Nn + Kn),
        ("W o A", J.compose(W, A), d, m, NKn + 2 * Nn + Kn),
        ("M' o A' o W o A o M", J.compose(J.compose(J.compose(J.compose(M.H, A.H), W), A), M), y, m, NKn + Nn + 4 * Kn),
    ):
        g0 = chains.STATS["grid_chain_calls"]
        ms_f, ms_u = ab(lambda: J.mul_(out, op, x), reps)
        ran = chains.STATS["grid_chain_calls"] > g0
        bw = nbytes / (ms_f * 1e-3)
        print(f"{tag:22s} fused {ms_f:9.3f} ms  {nbytes / 1e9:8.2f} GB  {bw / 1e12:5.2f} TB/s  {100 * bw / PEAK:5.1f} % of 8 TB/s   "
              f"stage by stage {ms_u:9.3f} ms   {ms_u / ms_f:5.2f}x   ({'grid chain ran' if ran else 'NOT FUSED'})", flush=True)
    if solvers:
        L = J.compose(W, A)
        b = J.rand(J.range(L), seed=9, stream=0)
        for name in ("cgnr", "lsqr"):
            fn = getattr(J, name)
            it = 10
            f, u = [], []
            for _ in range(2):
                chains.ENABLED[0] = True
                J.synchronize(); e0 = J.Event().record(); fn(L, b, maxiter=it, atol=0.0, btol=0.0, force_maxiter=True); e1 = J.Event().record()
                f.append(e0.elapsed_ms(e1) / it)
                chains.ENABLED[0] = False
                try:
                    J.synchronize(); e0 = J.Event().record(); fn(L, b, maxiter=it, atol=0.0, btol=0.0, force_maxiter=True); e1 = J.Event().record()
                    u.append(e0.elapsed_ms(e1) / it)
                finally:
                    chains.ENABLED[0] = True
            print(f"{name.upper() + ' on W o A':22s} fused {min(f):9.3f} ms/iteration   stage by stage {min(u):9.3f} ms/iteration   {min(u) / min(f):5.2f}x", flush=True)
    J.close(A)


if len(sys.argv) > 3:
    dt = {"f32": np.float32, "f64": np.float64, "c32": np.complex64, "c64": np.complex128}[sys.argv[4] if len(sys.argv) > 4 else "f32"]
    case(int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), dt)
else:
    case(64, 4, 256, solvers=True)
    case(128, 2, 256)
    case(64, 4, 255)
    case(4096, 3, 64)
    case(64, 4, 256, lam_rows=True)
