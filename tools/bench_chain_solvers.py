#!/usr/bin/env python3
"""LSQR / CGLS / CGNR per iteration on a weighted operator L = W o A, two routes, in ONE process, alternating in both orders:

  fused  the solvers on the FORWARD chain (jh_lsqr_solve_chain / jh_cgls_solve_chain / jh_cgnr_solve_chain: the one-pass chain step
         jh_chain_bidiag_step and the NORMAL program derived from the same handle)
  old    today's route without them: JETS_CHAIN_STEP=0 and JETS_*_NATIVE=0 -- the Python loop, the FORWARD chain into a range temporary, a
         lincomb and a norm over the range, then the ADJOINT chain (CGNR: A then A' through a range temporary)

A per-iteration time is (t(2K) - t(K)) / K of force_maxiter solves (the setup -- A'b, the copies of b -- cancels).  The two routes' x are
compared (relative difference).  `--fused-only` runs the fused route alone (sizes where the old route's range temporary does not fit:
1024 x 256^3 Float32 needs 64 GiB more for it), `--iters` the 100-iteration LSQR wall time of that route.

    python tools/bench_chain_solvers.py [--nrow 256] [--edge 256] [--k 10] [--solvers lsqr,cgls,cgnr] [--fused-only] [--iters 0]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NATIVE_ENV = {"lsqr": "JETS_LSQR_NATIVE", "cgls": "JETS_CGLS_NATIVE", "cgnr": "JETS_CGLS_NATIVE"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nrow", type=int, default=256)
    ap.add_argument("--edge", type=int, default=256)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--solvers", default="lsqr,cgls,cgnr")
    ap.add_argument("--fused-only", action="store_true")
    ap.add_argument("--iters", type=int, default=0, help="also time one solve of this many LSQR iterations on the fused route")
    args = ap.parse_args()

    import jets_jl_amd as J
    from jets_jl_amd import chains

    J.init(0)
    dt, nrow = np.float32, args.nrow
    spc = J.JetSpace(dt, args.edge, args.edge, args.edge)
    n = spc.length()
    A = J.blockop([[J.JopDiagonal(J.rand(spc, seed=1, stream=i))] for i in range(nrow)])
    W = J.JopDiagonal(J.rand(J.range(A), seed=2, stream=0))
    L = W @ A
    b = J.rand(J.range(A), seed=3, stream=0)
    s_bytes = 4
    fns = {"lsqr": J.lsqr, "cgls": J.cgls, "cgnr": J.cgnr}

    def set_route(route, solver):
        for v in ("JETS_CHAIN_STEP", "JETS_LSQR_NATIVE", "JETS_CGLS_NATIVE"):
            os.environ.pop(v, None)
        if route == "old":
            os.environ["JETS_CHAIN_STEP"] = "0"
            os.environ[NATIVE_ENV[solver]] = "0"

    def solve(route, solver, iters):
        set_route(route, solver)
        kw = dict(conlim=0.0) if solver == "lsqr" else {}
        if args.fused_only and solver != "cgnr":
            kw["overwrite_b"] = True                                   # (no private copy of b: at 1024 x 256^3 four range vectors do not fit)
        J.synchronize()
        t0 = time.perf_counter()
        res = fns[solver](L, b, atol=0.0, btol=0.0, maxiter=iters, force_maxiter=True, **kw)
        J.synchronize()
        return time.perf_counter() - t0, res

    out = {"shape": [nrow, args.edge, args.edge, args.edge], "dtype": "Float32", "k": args.k, "solvers": {}}
    routes = ["fused"] if args.fused_only else ["fused", "old"]
    for solver in args.solvers.split(","):
        times = {r: [] for r in routes}
        xs = {}
        s0 = dict(chains.STATS)
        orders = [routes, list(reversed(routes))] * 2
        for order in orders:
            for r in order:
                t1, _ = solve(r, solver, args.k)
                t2, res = solve(r, solver, 2 * args.k)
                times[r].append((t2 - t1) / args.k * 1e3)
                xs[r] = res.x.to_numpy().ravel(order="F")
        rec = {r: {"ms_per_iter": sorted(v), "median_ms": float(np.median(v))} for r, v in times.items()}
        if "old" in rec:
            rec["speedup"] = rec["old"]["median_ms"] / rec["fused"]["median_ms"]
            rec["x_rel_diff"] = float(np.linalg.norm(xs["fused"] - xs["old"]) / np.linalg.norm(xs["old"]))
        passes = {"lsqr": 4.0, "cgls": 6.0, "cgnr": 2.0}[solver]          # fused: step (A, W, u in, u out) ; + NORMAL (A, W) ; NORMAL only
        rec["fused"]["model_bytes_per_iter"] = passes * nrow * n * s_bytes
        rec["fused"]["tb_s_model"] = rec["fused"]["model_bytes_per_iter"] / (rec["fused"]["median_ms"] * 1e-3) / 1e12
        rec["stats"] = {k: chains.STATS[k] - s0[k] for k in ("chain_step_calls", "chain_solve_calls", "chain_calls")}
        out["solvers"][solver] = rec
        print(json.dumps({solver: rec}), flush=True)
    if args.iters:
        t, res = solve("fused", "lsqr", args.iters)
        out["lsqr_solve"] = {"iters": args.iters, "wall_s": t, "ms_per_iter_incl_setup": t / args.iters * 1e3, "itn": res.itn}
        print(json.dumps({"lsqr_solve": out["lsqr_solve"]}), flush=True)
    set_route("fused", "lsqr")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
