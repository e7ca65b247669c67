#!/usr/bin/env python3
"""A row shard whose local operator is a WEIGHTED N x K grid, L = W o A: the ranged one-pass grid-chain step and the solvers that iterate on the ranged
grid chains (knob grid_chain_range = 1 with grid_chain_step = 1: jh_chain_bidiag_step_range / jh_chain_apply_range over positions inside a block, the K
pieces of a finished range exchanged under the next range's kernel) against the route they replace (knob 0: both calls decline the grid chain, so a
step is the FORWARD grid chain into a range temporary, a range lincomb and norm, the ADJOINT grid chain and one unpipelined all-reduce of the domain
vector).  One rank, the exchange forced (BENCH_FORCE_DIST=1, AbiComm), JETS_AR_CHUNKS ranges; the two settings alternate in one process (knob 0 is the
default route: grid_chain_step goes to 0 with it, as in a process that sets neither knob).

    python tools/bench_grid_chain_range.py [nrow ncol edge [iters]] [--out FILE]        default: 64 x 4 of 256^3 Float32; FILE: profiles/bench_grid_chain_range.txt

Algorithmic bytes per step (s = element size, N x K blocks of n elements, NW = 1 weight): the ranged step (N K + (NW + 2) N + 2 K) n s, as the
unpartitioned one-pass chain step; the knob-0 route (2 N K + (2 NW + 6) N + 2 K) n s.  Also printed: the ranged step summed over its
ranges WITHOUT the exchange against the whole-vector jh_chain_bidiag_step, in the same process.  Every line is appended to FILE as well."""
import ctypes as C
import importlib
import os
import sys

os.environ["BENCH_FORCE_DIST"] = "1"
os.environ.setdefault("JETS_AR_CHUNKS", "4")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import jets_jl_amd as J
from jets_jl_amd import chains, rowpart
from jets_jl_amd._ffi import check, lib

_lsqr = importlib.import_module("jets_jl_amd.lsqr")     # (the package exports the solver under the module's name)

args = sys.argv[1:]
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "bench_grid_chain_range.txt")
if "--out" in args:
    at = args.index("--out")
    OUT = args[at + 1]
    del args[at:at + 2]
J.init(0)


def say(line):
    print(line, flush=True)
    with open(OUT, "a", encoding="utf-8") as f:
        f.write(line + "\n")


def timed(fn, reps):
    fn()
    J.synchronize()
    e0 = J.Event().record()
    for _ in range(reps):
        fn()
    e1 = J.Event().record()
    return e0.elapsed_ms(e1) / reps


def case(nrow, ncol, edge, iters=10, dt=np.float32):
    blk = J.JetSpace(dt, edge, edge, edge)
    n, s = blk.length(), np.dtype(dt).itemsize
    coeff = J.rand(J.JetBSpace([blk] * (nrow * ncol)), seed=1, stream=0)
    A = J.blockop([[J.JopDiagonal(coeff.arrays[i * ncol + k]) for k in range(ncol)] for i in range(nrow)])
    L = J.compose(J.JopDiagonal(J.rand(J.range(A), seed=4, stream=0)), A)
    new_b = (nrow * ncol + 3 * nrow + 2 * ncol) * n * s
    old_b = (2 * nrow * ncol + 8 * nrow + 2 * ncol) * n * s
    reps = max(3, int(4.0e10 / new_b))
    nchunks = int(os.environ["JETS_AR_CHUNKS"])
    say(f"# {nrow} x {ncol} of {edge}^3 {np.dtype(dt).name}, one rank, forced exchange, {nchunks} ranges: {nrow * ncol * n * s / 2**30:.1f} GiB of coefficients, one weight, "
        f"{reps} repetitions, byte ratio {old_b / new_b:.2f}")
    comm = rowpart.AbiComm(nranks=1, rank=0)
    # the knob-0 legs run on a shard and engines of their own, built with both knobs at their defaults: the route of a process that sets neither
    shards = {0: rowpart.for_device(rowpart.partition_rows(nrow, 1, 0), L, comm=comm)}
    assert not shards[0].chain_step and not shards[0].fused_normal
    J.tune(grid_chain_step=1, grid_chain_range=1)
    shards[1] = shard = rowpart.for_device(rowpart.partition_rows(nrow, 1, 0), L, comm=comm)
    sc = chains.SolverChains(L)
    h = sc.fwd
    assert h is not None and h.grid and shard.chain_step
    u = J.rand(J.range(A), seed=3, stream=0)
    v = J.rand(J.domain(A), seed=2, stream=0)
    w = J.zeros(J.domain(A))
    out = C.c_double(0)

    # the unpartitioned one-pass step, and the same step in ranges without the exchange
    def whole():
        check(lib.jh_chain_bidiag_step(h.handle, u.handle, v.handle, w.handle, 1.0, -0.5, C.byref(out)))

    def ranges():
        check(lib.jh_normsq_reset())
        for lo, cnt in rowpart._grid_chunk_bounds(n, nchunks):
            check(lib.jh_chain_bidiag_step_range(h.handle, u.handle, v.handle, w.handle, 1.0, -0.5, lo, cnt, None))
        check(lib.jh_normsq_read(C.byref(out)))

    J.tune(grid_chain_range=1, grid_chain_step=1)
    ms_w, ms_r = [], []
    for _ in range(3):
        ms_w.append(timed(whole, reps))
        ms_r.append(timed(ranges, reps))
    say(f"{'kernels':8s} whole-vector step {min(ms_w):9.3f} ms  {new_b / (min(ms_w) * 1e-3) / 1e12:5.2f} TB/s   in {nchunks} ranges {min(ms_r):9.3f} ms  "
        f"{new_b / (min(ms_r) * 1e-3) / 1e12:5.2f} TB/s   {100 * (min(ms_r) / min(ms_w) - 1):+5.1f} %")

    # the shard's step: what lsqr_core runs per iteration under either knob
    def shard_step():
        eng = engines[J.tune_get("grid_chain_range")]
        if eng.step(u, v, 1.0, -0.5) is None:
            eng.fwd(u, v, 1.0, -0.5)
            eng.adj(w, u, 1.0, 0.0)

    engines, f, o = {}, [], []
    for k in (1, 0):
        J.tune(grid_chain_range=k, grid_chain_step=k)
        engines[k] = _lsqr._ShardEngine(shards[k])
    for _ in range(3):
        for k, acc in ((1, f), (0, o)):
            J.tune(grid_chain_range=k, grid_chain_step=k)
            g0 = chains.STATS["grid_range_calls"]
            acc.append(timed(shard_step, reps))
            assert (chains.STATS["grid_range_calls"] > g0) == (k == 1), "the route is not the one the knob asks for"
    say(f"{'step':8s} grid_chain_range 1 {min(f):9.3f} ms  {new_b / 1e9:8.2f} GB  {new_b / (min(f) * 1e-3) / 1e12:5.2f} TB/s   "
        f"grid_chain_range 0 {min(o):9.3f} ms  {old_b / 1e9:8.2f} GB  {old_b / (min(o) * 1e-3) / 1e12:5.2f} TB/s   {min(o) / min(f):5.2f}x")
    del engines, u, w
    J.trim()
    b = J.rand(J.range(L), seed=9, stream=0)
    for name in ("lsqr", "cgls", "cgnr"):
        fn = getattr(J, name)
        f, o, xs = [], [], {}
        for _ in range(2):
            for k in (1, 0):
                J.tune(grid_chain_range=k, grid_chain_step=k)
                g0 = chains.STATS["grid_range_calls"]
                J.synchronize()
                e0 = J.Event().record()
                r = fn(shards[k], b, maxiter=iters, atol=0.0, btol=0.0, force_maxiter=True)
                e1 = J.Event().record()
                assert (chains.STATS["grid_range_calls"] > g0) == (k == 1), "the route is not the one the knob asks for"
                (f if k else o).append(e0.elapsed_ms(e1) / iters)
                xs[k] = r.x.to_numpy().ravel(order="F").astype(np.float64)
                del r
                J.trim()
        diff = np.linalg.norm(xs[1] - xs[0]) / np.linalg.norm(xs[0])
        say(f"{name.upper():8s} grid_chain_range 1 {min(f):9.3f} ms/iteration   grid_chain_range 0 {min(o):9.3f} ms/iteration   {min(o) / min(f):5.2f}x   "
            f"|x_1 - x_0| / |x_0| = {diff:.2e}")
    J.tune(grid_chain_range=0, grid_chain_step=0)
    sc.close()
    shards[0].close()
    shards[1].close()
    comm.close()
    J.close(A)


if len(args) >= 3:
    case(int(args[0]), int(args[1]), int(args[2]), int(args[3]) if len(args) > 3 else 10)
else:
    case(64, 4, 256)
