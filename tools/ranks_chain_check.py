#!/usr/bin/env python3
"""W processes drive WEIGHTED shards of the row partition (L = W_loc o A_loc) on the device and are checked against the CPU oracle (test
infrastructure; the plain shards' counterpart is tools/ranks_check.py).

    python tools/ranks_chain_check.py OUTDIR --ranks W --backend gloo     # W ranks on device 0, exchange staged through the host
    python tools/ranks_chain_check.py OUTDIR --ranks W --backend nccl     # one rank per GPU (needs >= W devices)

The launcher never touches the GPU: it spawns the ranks, waits, then loads the CPU oracle and compares.  Per rank, on ITS rows of the seeded
A and W (index_base slices of the counter generator, like bench.py): rowpart.for_device over torch.distributed with JETS_AR_CHUNKS=4 -- the
weighted adjoint and the weighted normal operator as ranged fused chains (jh_chain_apply_range), each range all-reduced behind its kernel --
and CG on the normal equations (cgls.cgnr: one NORMAL chain + the ranged exchange per iteration).
Checks: replicas bit-identical; adjoint and normal within rel-l2 1e-5 of the sequential fp64 result; CGNR within 1e-4 of the fp64 CPU CGLS of
oracle/cgls_ref.py on the whole weighted operator.
"""
import argparse
import os
import socket
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NROW_PER_RANK, SHAPE, CG_ITERS = 3, (64, 64, 20), 15      # 81 920 elements: three 64 KiB-aligned exchange ranges


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def nrow_for(world):
    return NROW_PER_RANK * world + 1          # uneven on purpose: rank 0 owns one row more


def _worker(rank, world, port, backend, out_dir):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    os.environ["JETS_AR_CHUNKS"] = "4"
    import torch
    import torch.distributed as dist

    device = rank if backend == "nccl" else 0
    if backend == "nccl":
        if torch.cuda.device_count() < world:
            raise SystemExit(f"--backend nccl needs {world} devices, {torch.cuda.device_count()} visible")
        torch.cuda.set_device(device)
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", device))
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    import jets_jl_amd as J
    from jets_jl_amd import chains

    J.init(device)
    dt = np.float32
    nrow, shape = nrow_for(world), SHAPE
    n = int(np.prod(shape))
    part = J.rowpart.partition_rows(nrow, world, rank)
    blk = J.JetSpace(dt, *shape)
    rsp = J.JetBSpace([blk] * part.count)

    def one_plus(x):                                                   # [1, 2): a well-conditioned weighted system
        return J.lincomb_(x, [1.0, 1.0], [x, J.ones(J.space(x))])

    coeff = one_plus(J.rand(rsp, seed=1, stream=0, index_base=part.first * n))
    A = J.blockop([[J.JopDiagonal(c)] for c in coeff.arrays])
    W = J.JopDiagonal(one_plus(J.rand(rsp, seed=6, stream=0, index_base=part.first * n)))     # this rank's rows of the weights
    L = W @ A
    m = J.rand(J.domain(A), seed=2, stream=0)
    d = J.rand(rsp, seed=3, stream=0, index_base=part.first * n)
    x_true = J.rand(J.domain(A), seed=4, stream=0)
    out = dict(first=part.first, count=part.count)

    shard = J.rowpart.for_device(part, L)
    before = chains.STATS["chain_range_calls"]
    out["mt"] = shard.mul_adj_(J.rand(J.domain(A), seed=9, stream=rank), d).to_numpy().ravel(order="F")        # dirty, rank-dependent buffer
    out["yn"] = shard.normal_mul_(J.rand(J.domain(A), seed=8, stream=rank), m).to_numpy().ravel(order="F")     # no tmp_local
    out["ranged"] = chains.STATS["chain_range_calls"] - before
    b = L * x_true
    res = J.cgnr(shard, b, atol=0.0, btol=0.0, maxiter=CG_ITERS)
    out["x"] = res.x.to_numpy().ravel(order="F")
    out["itn"] = res.itn
    shard.close()
    np.savez(os.path.join(out_dir, f"r{rank}.npz"), **out)
    dist.barrier()
    dist.destroy_process_group()


def check(out_dir, world):
    """Compare the ranks with the CPU oracle (test code: loads oracle/)."""
    sys.path.insert(0, ROOT)
    from oracle import jets_oracle as oracle
    from oracle.cgls_ref import cgls_fp64

    nrow, shape = nrow_for(world), SHAPE
    n = int(np.prod(shape))
    res = [np.load(os.path.join(out_dir, f"r{r}.npz")) for r in range(world)]
    dt = np.float32
    a = np.stack([oracle.rng_u01(dt, 1, 0, i * n, n) + dt(1) for i in range(nrow)]).astype(np.float64)
    w = np.stack([oracle.rng_u01(dt, 6, 0, i * n, n) + dt(1) for i in range(nrow)]).astype(np.float64)
    m = oracle.rng_u01(dt, 2, 0, 0, n).astype(np.float64)
    d = np.stack([oracle.rng_u01(dt, 3, 0, i * n, n) for i in range(nrow)]).astype(np.float64)
    hx = oracle.rng_u01(dt, 4, 0, 0, n)
    counts = [int(r["count"]) for r in res]
    assert sum(counts) == nrow and [int(r["first"]) for r in res] == list(np.cumsum([0] + counts[:-1])), f"partition {counts}"
    for r in res:
        assert int(r["ranged"]) == 6, f"ranged chain calls {int(r['ranged'])}: three for the adjoint, three for the normal operator"
    ref = {"mt": (a * w * d).sum(0), "yn": (a * w * w * a * m).sum(0)}
    for key, want in ref.items():
        for r in res[1:]:
            assert r[key].tobytes() == res[0][key].tobytes(), f"{key}: replicas differ"
        err = np.linalg.norm(res[0][key].astype(np.float64) - want) / np.linalg.norm(want)
        assert err <= 1e-5, f"{key}: rel-l2 {err:.2e} vs the sequential fp64 result"
    aw32 = (np.stack([oracle.rng_u01(dt, 6, 0, i * n, n) + dt(1) for i in range(nrow)]) *
            (np.stack([oracle.rng_u01(dt, 1, 0, i * n, n) + dt(1) for i in range(nrow)]) * hx[None, :]))
    b64 = aw32.astype(np.float64).ravel()                              # b = W (A x_true): the Float32 products, like the device's
    aw = a * w
    xr, _ = cgls_fp64(lambda v: (aw * v[None, :]).ravel(), lambda u: (aw * u.reshape(nrow, n)).sum(axis=0), b64, n, damp=0.0, atol=0.0, btol=0.0,
                      maxiter=CG_ITERS)
    for r in res[1:]:
        assert r["x"].tobytes() == res[0]["x"].tobytes(), "CGNR: replicas differ"
    assert int(res[0]["itn"]) == CG_ITERS
    err = np.linalg.norm(res[0]["x"].astype(np.float64) - xr) / np.linalg.norm(xr)
    assert err <= 1e-4, f"CGNR: rel-l2 {err:.2e} vs the fp64 CPU CGLS"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--ranks", type=int, default=2)
    ap.add_argument("--backend", default="gloo", choices=["nccl", "gloo"])
    args = ap.parse_args()
    import torch.multiprocessing as mp

    os.makedirs(args.out, exist_ok=True)
    t0 = time.time()
    mp.spawn(_worker, args=(args.ranks, _free_port(), args.backend, args.out), nprocs=args.ranks, join=True)
    check(args.out, args.ranks)
    print(f"{args.ranks} ranks over {args.backend}: {time.time() - t0:.1f} s", flush=True)
    print("RANKS CHAINS OK", flush=True)


if __name__ == "__main__":
    main()
