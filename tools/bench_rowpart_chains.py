#!/usr/bin/env python3
"""The weighted normal operator of a row-partitioned shard, three ways, in ONE process, alternating (config 3w's operator on a shard):

  (a) whole   the whole-vector fused NORMAL chain A' o W' o W o A (jh_chain_apply) -- one GPU, no exchange: the floor
  (b) ranged  the weighted shard's normal_mul_: the NORMAL chain in 4 element ranges (jh_chain_apply_range), each range all-reduced
              (jh_comm_allreduce_sum_range) behind its kernel, then jh_comm_join
  (c) before  the route a weighted shard took before it had (b): forward chain W o A into a range temporary, adjoint chain (W o A)',
              one whole all-reduce

One rank (AbiComm(nranks=1)) with the collective forced, 256 x 256^3 Float32 with range weights W.  The outputs of (a), (b), (c) are
compared.  Times are HIP events on the library stream around one application (the ranged route's stop event is behind jh_comm_join).

    python tools/bench_rowpart_chains.py [--reps 20] [--warmup 3] [--only b]      # --only: one route (a profiler run of it)
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--nrow", type=int, default=256)
    ap.add_argument("--edge", type=int, default=256)
    ap.add_argument("--only", choices=["a", "b", "c"], default=None)
    args = ap.parse_args()
    os.environ.setdefault("JETS_AR_CHUNKS", "4")

    import jets_jl_amd as J
    from jets_jl_amd import chains

    J.init(0)
    dt, nrow = np.float32, args.nrow
    spc = J.JetSpace(dt, args.edge, args.edge, args.edge)
    n = spc.length()
    A = J.blockop([[J.JopDiagonal(J.rand(spc, seed=1, stream=i))] for i in range(nrow)])
    W = J.JopDiagonal(J.rand(J.range(A), seed=2, stream=0))
    L = W @ A
    N = L.H @ L
    m = J.rand(J.domain(A), seed=3, stream=0)
    comm = J.rowpart.AbiComm(nranks=1, rank=0)
    shard = J.rowpart.for_device(J.rowpart.partition_rows(nrow, 1, 0), L, comm=comm)
    ys = {k: J.zeros(J.domain(A)) for k in "abc"}
    tmp = J.zeros(J.range(A)) if args.only in (None, "c") else None

    def run(k):
        y = ys[k]
        if k == "a":
            J.mul_(y, N, m)
        elif k == "b":
            shard.normal_mul_(y, m, force_collective=True)
        else:
            shard.mul_(tmp, m)
            J.mul_(y, L.H, tmp)
            comm.all_reduce_sum_(y, force=True)

    routes = [args.only] if args.only else ["a", "b", "c"]
    times = {k: [] for k in routes}
    r0 = chains.STATS["chain_range_calls"]
    for it in range(args.warmup + args.reps):
        for k in (routes if it % 2 == 0 else routes[::-1]):             # alternating, both orders
            e0 = J.Event().record()
            run(k)
            e1 = J.Event().record()
            J.synchronize()
            if it >= args.warmup:
                times[k].append(e0.elapsed_ms(e1))
    ranged = chains.STATS["chain_range_calls"] - r0
    bytes_streamed = 2.0 * nrow * n * 4                                     # A and W once: the NORMAL chain's traffic (+ the domain vectors)
    out = {"tool": "bench_rowpart_chains", "nrow": nrow, "n": n, "dtype": "Float32", "reps": args.reps, "chunks": int(os.environ["JETS_AR_CHUNKS"]),
           "ranged_calls": ranged, "device": J.device_info()["name"]}
    for k in routes:
        t = np.array(times[k])
        out[f"{k}_ms_median"] = round(float(np.median(t)), 4)
        out[f"{k}_ms_min"] = round(float(t.min()), 4)
        out[f"{k}_ms_max"] = round(float(t.max()), 4)
        out[f"{k}_tb_s_at_2Nns"] = round(bytes_streamed / (float(np.median(t)) * 1e-3) / 1e12, 3)
    if "a" in routes and "b" in routes:
        out["b_over_a"] = round(out["b_ms_median"] / out["a_ms_median"], 4)
    if "a" in routes and "c" in routes:
        out["c_over_a"] = round(out["c_ms_median"] / out["a_ms_median"], 4)
    if len(routes) == 3:
        ya, yb, yc = (ys[k].to_numpy().ravel(order="F") for k in "abc")
        out["b_equals_a_bitwise"] = bool(ya.tobytes() == yb.tobytes())
        out["c_equals_a_bitwise"] = bool(ya.tobytes() == yc.tobytes())
        den = float(np.abs(ya).max())
        out["max_rel_diff_b"] = float(np.abs(yb.astype(np.float64) - ya).max() / den)
        out["max_rel_diff_c"] = float(np.abs(yc.astype(np.float64) - ya).max() / den)
    print(json.dumps(out), flush=True)
    shard.close()
    comm.close()


if __name__ == "__main__":
    main()
