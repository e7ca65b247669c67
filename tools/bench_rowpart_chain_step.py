#!/usr/bin/env python3
"""LSQR and CGLS on a WEIGHTED row-partitioned shard, per iteration, two routes alternating in ONE process:

  new     the ranged one-pass chain step (jh_chain_bidiag_step_range, JETS_AR_CHUNKS ranges, each range's all-reduce of w under the next range's
          kernel; CGLS: the ranged NORMAL chain, then that step) -- no range-sized temporary
  before  JETS_CHAIN_STEP=0: the FORWARD chain into a range temporary, a range lincomb and a norm, the ranged ADJOINT chain

One GPU, one rank (AbiComm(nranks=1)) with the exchange forced (BENCH_FORCE_DIST=1), Float32 W o A with the weights in one slab.  A solve of K
iterations is timed with HIP events on the library stream; the per-iteration figure is (t(K2) - t(K1)) / (K2 - K1), which drops the set-up passes.
Also: one step with its exchange against the same ranged kernels without it -- the exposed part of the exchange (the last range's all-reduce and
the join) -- for the weighted shard and, beside it, for the bare block operator's step (jh_blockop_bidiag_step_range).

    python tools/bench_rowpart_chain_step.py [--nrow 256] [--edge 256] [--reps 5]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--nrow", type=int, default=256)
    ap.add_argument("--edge", type=int, default=256)
    ap.add_argument("--k1", type=int, default=2)
    ap.add_argument("--k2", type=int, default=10)
    args = ap.parse_args()
    os.environ.setdefault("JETS_AR_CHUNKS", "4")
    os.environ["BENCH_FORCE_DIST"] = "1"

    import jets_jl_amd as J
    from jets_jl_amd import chains, jetblock, rowpart
    from jets_jl_amd._ffi import check, lib

    J.init(0)
    dt, nrow = np.float32, args.nrow
    spc = J.JetSpace(dt, args.edge, args.edge, args.edge)
    n = spc.length()

    def one_plus(x):
        return J.lincomb_(x, [1.0, 1.0], [x, J.ones(J.space(x))])

    A = J.blockop([[J.JopDiagonal(one_plus(J.rand(spc, seed=1, stream=i)))] for i in range(nrow)])
    L = J.JopDiagonal(one_plus(J.rand(J.range(A), seed=2, stream=0))) @ A
    b = J.rand(J.range(A), seed=3, stream=0)
    comm = rowpart.AbiComm(nranks=1, rank=0)
    part = rowpart.partition_rows(nrow, 1, 0)

    def shard_for(op, route):
        os.environ["JETS_CHAIN_STEP"] = "1" if route == "new" else "0"
        return rowpart.for_device(part, op, comm=comm)

    def timed(fn):
        e0 = J.Event().record()
        r = fn()
        e1 = J.Event().record()
        J.synchronize()
        return e0.elapsed_ms(e1), r

    out = {"tool": "bench_rowpart_chain_step", "nrow": nrow, "n": n, "dtype": "Float32", "reps": args.reps, "chunks": int(os.environ["JETS_AR_CHUNKS"]),
           "k1": args.k1, "k2": args.k2, "device": J.device_info()["name"]}
    for solver in ("lsqr", "cgls"):
        solve = getattr(J, solver)
        per = {"new": [], "before": []}
        for rep in range(args.reps + 1):                                     # (rep 0: warm-up -- plans, handles, the slab cache)
            for route in (("new", "before") if rep % 2 == 0 else ("before", "new")):
                shard = shard_for(L, route)
                s0 = chains.STATS["chain_step_range_calls"]
                ts = {}
                for k in (args.k1, args.k2):
                    ts[k], res = timed(lambda: solve(shard, b, atol=0.0, btol=0.0, maxiter=k, force_maxiter=True))
                    assert res.itn == k, (solver, route, res.itn, res.istop)
                    del res
                steps = chains.STATS["chain_step_range_calls"] - s0
                assert (steps > 0) == (route == "new"), (route, steps)
                shard.close()
                if rep > 0:
                    per[route].append((ts[args.k2] - ts[args.k1]) / (args.k2 - args.k1))
        for route in per:
            t = np.array(per[route])
            out[f"{solver}_{route}_ms_per_iter"] = [round(float(x), 3) for x in t]
            out[f"{solver}_{route}_ms_median"] = round(float(np.median(t)), 3)
        out[f"{solver}_speedup"] = round(out[f"{solver}_before_ms_median"] / out[f"{solver}_new_ms_median"], 3)

    # one step: with its exchange, and the same ranged kernels alone (the difference is the exposed part of the exchange)
    os.environ["JETS_CHAIN_STEP"] = "1"
    u = J.copyto_(J.zeros(J.range(A)), b)
    v, w = J.rand(J.domain(A), seed=4, stream=0), J.zeros(J.domain(A))
    bounds = list(rowpart._chunk_bounds(n, int(os.environ["JETS_AR_CHUNKS"])))
    nsq = C.c_double(0)
    for tag, op in (("chain", L), ("blockop", A)):
        shard = shard_for(op, "new")
        if tag == "chain":
            h = shard._chains.step()
            kern = lambda lo, cnt: h.bidiag_step_range(u, v, w, 1.0, -0.5, lo, cnt)
        else:
            nat = jetblock._tall_native(A)
            kern = lambda lo, cnt: check(lib.jh_blockop_bidiag_step_range(nat.handle, u.handle, v.handle, w.handle, 1.0, -0.5, lo, cnt, None))

        def alone():
            check(lib.jh_normsq_reset())
            for lo, cnt in bounds:
                kern(lo, cnt)
            check(lib.jh_normsq_read(C.byref(nsq)))

        with_x, without = [], []
        for rep in range(args.reps + 2):
            for which in ((0, 1) if rep % 2 == 0 else (1, 0)):
                t, _ = timed((lambda: shard.bidiag_step_(u, v, w, 1.0, -0.5, force_collective=True)) if which == 0 else alone)
                if rep >= 2:
                    (with_x if which == 0 else without).append(t)
        out[f"{tag}_step_with_exchange_ms"] = [round(x, 3) for x in with_x]
        out[f"{tag}_step_kernels_only_ms"] = [round(x, 3) for x in without]
        out[f"{tag}_step_exposed_exchange_ms"] = round(float(np.median(with_x) - np.median(without)), 3)
        shard.close()
    print(json.dumps(out), flush=True)
    comm.close()


if __name__ == "__main__":
    main()
